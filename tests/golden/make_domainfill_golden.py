"""Regenerates tests/golden/bc_r4.npz and bc_r8.npz: what the reference's own boundcond_domainfill leaves behind after each of
DF_CALLS consecutive calls on the cases of flexpart_amd.synthetic.domainfill_case(), and the bytes of boundcond.bin.

The reference sources are compiled where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind with
-fdefault-real-8) together with our driver tests/golden/ref_bc_driver.f90 into a build directory outside git (a temporary
one unless --build-dir is given); nothing of the reference is copied or written anywhere.  The fixtures hold outputs only;
the inputs are regenerated bit for bit by the tests.  boundcond.bin has par_mod's extents (nxmax, nymax, maxcolumn: read from
the fixture as `par`), 26 MB in r4 that are almost all zeros: the fixtures are compressed.

    python tests/golden/make_domainfill_golden.py
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF = os.path.join(os.environ.get("FLEXPART_REFERENCE", "/root/reference"), "src")
FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
SOURCES = ("par_mod", "com_mod", "point_mod", "random_mod", "boundcond_domainfill")
INT_ARRAYS = ("itra1", "itramem", "npoint", "nclass", "idt", "itrasplit")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def par_extents():
    """nxmax, nymax, maxcolumn, maxpart of the reference's par_mod (the active, uncommented parameter statements)."""
    out = {}
    for line in open(os.path.join(REF, "par_mod.f90")):
        if line.lstrip().startswith("!"):
            continue
        for name in ("nxmax", "nymax", "maxcolumn", "maxpart"):
            m = re.search(r"\b%s\s*=\s*(\d+)" % name, line)
            if m and "parameter" in line:
                out[name] = int(m.group(1))
    return out


def build(kind, build_dir):
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"bcref_{kind}")
    drv = os.path.join(HERE, "ref_bc_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    objs = []
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_bc_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_bc_driver.o"] + objs[::-1] + ["-o", exe], cwd=d)
    return exe


def write_input(c, ncalls, fin):
    nx, ny, nz = (int(v) for v in c["grid"])
    cap = int(c["npart"])
    mc = int(np.asarray(c["zcolumn_we"]).shape[0])
    g = c["geom"]
    with open(fin, "wb") as f:
        np.array([nx, ny, nz, cap, c["numpart"], c["numparticlecount"], ncalls, c["itime"], c["lsynctime"], c["memind"][0], c["memind"][1],
                  c["memtime"][0], c["memtime"][1], c["mdomainfill"], c["globalflags"][0], c["gdomainfill"], c["nx_we"][0], c["nx_we"][1],
                  c["ny_sn"][0], c["ny_sn"][1], c["mintime"], c["ldirect"], c["itsplit"], mc], np.int32).tofile(f)
        np.array([g[0], g[1], g[3], c["xmassperparticle"]], np.float64).tofile(f)
        np.asarray(c["height"], np.float64).tofile(f)
        for m in range(2):
            for k in ("uu", "vv", "rho", "pv"):
                np.ascontiguousarray(c[k][m], np.float64).tofile(f)        # [kz][jy][ix] = Fortran (ix,jy,kz)
        np.ascontiguousarray(c["numcolumn_we"], np.int32).tofile(f)         # [row][k] = Fortran (k,row)
        np.ascontiguousarray(c["numcolumn_sn"], np.int32).tofile(f)
        for k in ("zcolumn_we", "zcolumn_sn", "acc_mass_we", "acc_mass_sn"):
            np.ascontiguousarray(c[k], np.float64).tofile(f)                # [j][row][k] = Fortran (k,row,j)
        for k in ("xtra1", "ytra1", "ztra1"):
            np.asarray(c[k], np.float64).tofile(f)
        np.asarray(c["xmass1"], np.float64)[0].tofile(f)
        for k in INT_ARRAYS:
            np.asarray(c[k], np.int32).tofile(f)


def read_output(c, kind, fout):
    """The calls the reference completed: a list of dicts."""
    rt = np.float32 if kind == "r4" else np.float64
    nx, ny, _ = (int(v) for v in c["grid"])
    cap = int(c["npart"])
    mc = int(np.asarray(c["zcolumn_we"]).shape[0])
    data = open(fout, "rb").read()
    rs = np.dtype(rt).itemsize
    per = 8 + 6 * 4 * cap + 2 * 8 * cap + 2 * rs * cap + 2 * (ny + nx) * mc * rs
    calls = []
    for i in range(len(data) // per):
        b = data[i * per:(i + 1) * per]
        o = 0

        def take(dtype, n):
            nonlocal o
            a = np.frombuffer(b, dtype, n, o).copy()
            o += a.nbytes
            return a
        r = {}
        r["numpart"], r["numparticlecount"] = (int(v) for v in take(np.int32, 2))
        for k in INT_ARRAYS:
            r[k] = take(np.int32, cap)
        r["xtra1"], r["ytra1"] = take(np.float64, cap), take(np.float64, cap)
        r["ztra1"], r["xmass1"] = take(rt, cap), take(rt, cap)
        r["acc_mass_we"] = take(rt, 2 * ny * mc).reshape(mc, ny, 2)
        r["acc_mass_sn"] = take(rt, 2 * nx * mc).reshape(mc, nx, 2)
        calls.append(r)
    return calls


def run(exe, c, kind, ncalls, workdir):
    """(completed calls, exit status, bytes of boundcond.bin or None)."""
    fin, fout = os.path.join(workdir, "bc_in.bin"), os.path.join(workdir, "bc_out.bin")
    fbin = os.path.join(workdir, "boundcond.bin")
    for p in (fout, fbin):
        if os.path.exists(p):
            os.remove(p)
    write_input(c, ncalls, fin)
    rc = subprocess.call([exe, fin, fout, workdir + os.sep], stdout=subprocess.DEVNULL)
    calls = read_output(c, kind, fout) if os.path.exists(fout) else []
    data = open(fbin, "rb").read() if os.path.exists(fbin) else None
    return calls, rc, data


def main():
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="bcref_")
    par = par_extents()
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {"par": np.array([par["nxmax"], par["nymax"], par["maxcolumn"]], np.int32)}
        for v in syn.DF_VARIANTS:
            c = syn.domainfill_case(v)
            calls, rc, data = run(exe, c, kind, syn.DF_CALLS, os.path.join(bd, kind))
            rec[f"{v}_status"] = np.array([rc, len(calls)], np.int32)
            for i, r in enumerate(calls):
                for k, val in r.items():
                    rec[f"{v}_{i}_{k}"] = np.asarray(val)
            if data is not None and v in ("fill1", "fill2", "xglobal"):
                rec[f"{v}_bin"] = np.frombuffer(data, np.uint8)
            print(kind, v, "status", rc, "calls", len(calls), "boundcond.bin", None if data is None else len(data))
        out = os.path.join(HERE, f"bc_{kind}.npz")
        np.savez_compressed(out, **rec)
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
