"""Regenerates tests/golden/pa_r4.npz and pa_r8.npz: npart_av and the fourteen sums before each output call and the
partposit_average_* files that the reference's own partpos_average and partoutput_average produce for
flexpart_amd.synthetic.partavg_case().

The reference sources (par_mod, com_mod, caldate, partpos_average, partoutput_average) are compiled where they lie with
flang (-cpp -O2 -mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver
tests/golden/ref_pa_driver.f90 into a build directory outside git (a temporary one unless --build-dir is given).  One
compile-time line differs from the shipped par_mod: the field extents nxmax, nymax, nzmax are 361 x 181 x 138 there, and
the `jyp >= nymax` fix-up of partpos_average.f90:56-59 is reached only by a particle on row nymax - 1, so the case's
20 x 12 x 10 grid needs nymax = 12.  As make_calcfluxes_golden.py does for maxageclass, par_mod is piped through that
one-line edit into the compiler; nothing of the reference is copied or written anywhere.  The fixtures hold results only;
the inputs are regenerated bit for bit by the tests.

    python tests/golden/make_partavg_golden.py
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
SOURCES = ("par_mod", "com_mod", "caldate", "partpos_average", "partoutput_average")
SIZES = ("integer,parameter :: nxmax=361,nymax=181,nuvzmax=138,nwzmax=138,nzmax=138\n",
         "integer,parameter :: nxmax=20,nymax=12,nuvzmax=10,nwzmax=10,nzmax=10\n")
SUMS = ("cartx", "carty", "cartz", "z", "topo", "pv", "qv", "tt", "uu", "vv", "rho", "tro", "hmix", "energy")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """paref_<kind> in build_dir (built once: an existing binary newer than the driver is kept)."""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"paref_{kind}")
    drv = os.path.join(HERE, "ref_pa_driver.f90")
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
                sys.exit("par_mod has no 'nxmax=361,nymax=181,...' line")
            subprocess.run([FC, "-c"] + flags + ["-x", "f95-cpp-input", "-", "-o", s + ".o"], cwd=d, check=True,
                           input=text.replace(SIZES[0], SIZES[1]).encode())
        else:
            subprocess.check_call([FC, "-c"] + flags + [src, "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_pa_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_pa_driver.o"] + objs[::-1] + ["-o", exe], cwd=d)
    return exe


def run(exe, c, workdir):
    """One pass of the driver over synthetic.partavg_case(): per output interval (dict of npart_av and the fourteen sums as
    float64, the bytes of the partposit_average file, its name)."""
    nx, ny, nz = (int(v) for v in c["grid"])
    n = int(c["npart"])
    out = os.path.join(workdir, "out")
    os.makedirs(out, exist_ok=True)
    for f in glob.glob(os.path.join(out, "partposit_average_*")):
        os.remove(f)
    fin, fout = os.path.join(workdir, "pa_in.bin"), os.path.join(workdir, "pa_out.bin")
    with open(fin, "wb") as f:
        np.array([nx, ny, nz, n, len(c["calls"])], np.int32).tofile(f)
        np.array(list(c["memtime"]) + list(c["memind"][:2]), np.int32).tofile(f)
        np.array([len(t) for t in c["calls"]], np.int32).tofile(f)
        np.array(c["outputs"], np.int32).tofile(f)
        np.array(list(c["geom"]) + [c["bdate"]], np.float64).tofile(f)
        np.asarray(c["height"], np.float64).tofile(f)
        np.ascontiguousarray(c["oro"], np.float64).tofile(f)              # [jy][ix] = Fortran (ix,jy)
        for m in range(2):
            for k in ("pv", "qv", "tt", "uu", "vv", "rho", "tropopause", "hmix"):
                np.ascontiguousarray(c[k][m], np.float64).tofile(f)
        ncall = 0
        for iv, times in enumerate(c["calls"]):
            for itime in times:
                np.array([itime], np.int32).tofile(f)
                for k in ("xt", "yt", "zt"):
                    np.asarray(c[f"{k}{ncall}"], np.float64).tofile(f)
                np.asarray(c[f"due{ncall}"], np.int32).tofile(f)
                ncall += 1
            np.asarray(c[f"itra1_{iv}"], np.int32).tofile(f)
    subprocess.check_call([exe, fin, fout, out + os.sep])
    res = []
    import partavg_ref as pr
    with open(fout, "rb") as f:
        for iv in range(len(c["calls"])):
            st = {"npart_av": np.fromfile(f, np.int32, n)}
            for k in SUMS:
                st[k] = np.fromfile(f, np.float64, n)
            name = pr.file_name(c["bdate"], c["outputs"][iv])
            path = os.path.join(out, name)
            res.append((st, open(path, "rb").read(), name))
    assert len(glob.glob(os.path.join(out, "partposit_average_*"))) == len(res)
    return res


def main():
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="paref_")
    c = syn.partavg_case()
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {}
        for iv, (st, data, name) in enumerate(run(exe, c, os.path.join(bd, kind))):
            rec[f"npart_av_{iv}"] = st["npart_av"]
            for k in SUMS:
                rec[f"{k}_{iv}"] = st[k].astype(np.float32 if kind == "r4" else np.float64)
            rec[f"file_{iv}"] = np.frombuffer(data, np.uint8)
            rec[f"name_{iv}"] = np.array(name)
        np.savez_compressed(os.path.join(HERE, f"pa_{kind}.npz"), **rec)
        print("wrote", f"pa_{kind}.npz", os.path.getsize(os.path.join(HERE, f"pa_{kind}.npz")), "bytes")


if __name__ == "__main__":
    main()
