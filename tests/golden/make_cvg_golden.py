"""Regenerates tests/golden/cvg_<case>_<kind>.npz -- what the reference's own convmix leaves with metdata_format =
GRIBFILE_CENTRE_NCEP on the cases of tests/convmix_gfs_ref.py (synthetic.convection_case_gfs: grid 24 x 16, 4000 particles, a
tenth not due; forward nz = 26, backward nz = 31, terrain nz = 34, deep nz = 26).

The unmodified reference sources par_mod, com_mod, conv_mod, flux_mod, outg_mod, random_mod, convmix, calcmatrix, convect43c,
redist, sort2, qvsat, ew, calcfluxes are compiled where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind with
-fdefault-real-8) together with our stand-in for class_gribfile (class_gribfile_standin.f90) and our driver
ref_cvg_driver.f90, into a build directory outside git (a temporary one unless --build-dir is given).  Nothing of the reference
is copied; the fixtures hold outputs only (the tests regenerate the synthetic inputs bit for bit).

Mode A, end to end: three consecutive calls of convmix one lsynctime apart: ztra1_<i>, cbaseflux_<i> after call i.
Mode B, per column, from the start state: for every column that holds due particles, convmix on the particles of that column
alone (cbaseflux restored afterwards): cols, lconv, nconvtop, exit, psconv, cbnew, pconv [m][nuvz] (pconv(nuvz) as the flang
build holds it), phconv [m][nuvz], dpr, tconv, qconv [m][nuvz-1].  The matrices are kept for the convective columns only
(fm_cols: their positions in cols; fmassfrac [mc][nconvlev+1][nconvlev+1], (k, kk) at [kk-1][k-1]; the driver checks that every
other column's matrix is zero, which is how lconv is read).  r4 values are exact in float32 and are stored so.

Before anything is written the script asserts, for every case and kind: at least 40 convective and 40 non-convective visited
columns; every exit of CONVECT before its mixing part that can be reached occurs (see EXIT 3 below); nconvtop <= nconvlev
everywhere -- except in the case `deep`, which is there for the opposite: some of its columns must reach nconvtop = nconvlev + 1
= nuvz - 1, where redist.f90:74-85 reads pconv, tconv, qconv and phconv at level nuvz, written by no GFS run (mode A's ztra1
then records what the reference makes of its static zeros); pconv(nuvz) = 0 in the flang build; the numpy restatement of the sounding equals the reference bit for bit; and
`noflip` of tests/convmix_gfs_ref.py holds.

EXIT 3 (iflag = 3, cloud base at nl-1 or above) cannot be reached on GFS levels, by CONVECT's own logic: it needs no level i in
nk+1 .. nl-2 with pconv(i) < plcl, while the exit before it has established plcl >= 200 hPa and level nl-2 = 22 lies at 70 hPa
(nl = nconvlev = 24 on the classic GFS levels; level 24 is 30 hPa); so nk = nl-2 = ihmin, and a level cannot be both the maximum of hm(1 .. ihmin) and below its predecessor.  The script asserts
that it does not occur instead.

    python tests/golden/make_cvg_golden.py            # writes the six fixtures
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
MODULES = ("par_mod", "com_mod", "conv_mod", "flux_mod", "outg_mod", "random_mod")
SOURCES = ("convmix", "calcmatrix", "convect43c", "redist", "sort2", "qvsat", "ew", "calcfluxes")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """cvgref_<kind> in build_dir/<kind> (an existing binary newer than the driver is kept)"""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"cvgref_{kind}")
    drv = os.path.join(HERE, "ref_cvg_driver.f90")
    standin = os.path.join(HERE, "class_gribfile_standin.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(drv), os.path.getmtime(standin)):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    for s in MODULES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
    subprocess.check_call([FC, "-c"] + flags + [standin, "-o", "class_gribfile.o"], cwd=d)
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_cvg_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_cvg_driver.o", "class_gribfile.o"] + [s + ".o" for s in SOURCES + MODULES[::-1]] + ["-o", exe], cwd=d)
    return exe


def _raise_stack():
    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def write_input(path, cs):
    """the driver's input file (also read by tests/convmix_gfs_host.cpp)"""
    nx, ny, nz = (int(v) for v in cs["grid"])
    n, ncalls = int(cs["npart"]), len(cs["itimes"])
    with open(path, "wb") as f:
        np.array([nx, ny, nz, int(cs["nconvlev"]), int(cs["ldirect"]), int(cs["lsynctime"]), int(cs["memtime"][0]), int(cs["memtime"][1]), n, ncalls],
                 np.int32).tofile(f)
        np.array([cs["height_nz"]], np.float64).tofile(f)
        for k in ("ps", "tt2", "td2", "tt", "qv", "pplev", "cbaseflux", "xtra1", "ytra1", "ztra1"):
            np.ascontiguousarray(cs[k], np.float64).tofile(f)
        np.ascontiguousarray(cs["itimes"], np.int32).tofile(f)
        np.ascontiguousarray(np.asarray(cs["due"]).T.astype(np.int32)).tofile(f)


def read_output(path, cs):
    nx, ny, nuvz = (int(v) for v in cs["grid"])
    n, ncalls, nl1 = int(cs["npart"]), len(cs["itimes"]), int(cs["nconvlev"]) + 1
    rec = {}
    with open(path, "rb") as f:
        for i in range(ncalls):
            rec[f"ztra1_{i}"] = np.fromfile(f, np.float64, n)
            rec[f"cbaseflux_{i}"] = np.fromfile(f, np.float64, nx * ny).reshape(ny, nx)
        m = int(np.fromfile(f, np.int32, 1)[0])
        ints = np.zeros((m, 4), np.int32)
        b = {k: [] for k in ("psconv", "cbnew", "pconv", "phconv", "dpr", "tconv", "qconv", "fmassfrac")}
        for c in range(m):
            ints[c] = np.fromfile(f, np.int32, 4)
            ps, cb = np.fromfile(f, np.float64, 2)
            b["psconv"].append(ps); b["cbnew"].append(cb)
            for k, cnt in (("pconv", nuvz), ("phconv", nuvz), ("dpr", nuvz - 1), ("tconv", nuvz - 1), ("qconv", nuvz - 1)):
                b[k].append(np.fromfile(f, np.float64, cnt))
            b["fmassfrac"].append(np.fromfile(f, np.float64, nl1 * nl1).reshape(nl1, nl1))
        assert f.read(1) == b""
    rec.update(cols=ints[:, 0].copy(), lconv=ints[:, 1].copy(), nconvtop=ints[:, 2].copy(), exit=ints[:, 3].copy())
    rec.update({k: np.array(v) for k, v in b.items()})
    return rec


def run(exe, cs, workdir):
    fin, fout = os.path.join(workdir, "cvg_in.bin"), os.path.join(workdir, "cvg_out.bin")
    write_input(fin, cs)
    log = subprocess.check_output([exe, fin, fout], text=True, preexec_fn=_raise_stack)
    return read_output(fout, cs), log


def main():
    import convmix_gfs_ref as gr
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="cvgref_")
    todo = {}
    for kind in gr.KINDS:
        store = np.float32 if kind == "r4" else np.float64
        exe = build(kind, bd)
        for name in gr.CASES:
            cs = gr.case(name)
            rec, log = run(exe, cs, bd)
            print(f"{name} {kind}: " + " | ".join(log.strip().splitlines()))
            cols, lc, nt, ex = rec["cols"], rec["lconv"], rec["nconvtop"], rec["exit"]
            assert np.array_equal(cols, gr.visited_columns(cs, 0)), (name, kind)
            nconv, nnot = int((lc == 1).sum()), int((lc == 0).sum())
            counts = {e: int((ex == e).sum()) for e in range(6)}
            print(f"  {len(cols)} visited columns, {nconv} convective, {nnot} not; exits {counts}; nconvtop {nt[lc == 1].min()} .. {nt.max()} "
                  f"(nconvlev {int(cs['nconvlev'])})")
            assert nconv >= 40 and nnot >= 40, (name, kind, nconv, nnot)
            assert counts[1] > 0 and counts[2] > 0 and counts[4] > 0 and counts[3] == 0, (name, kind, counts)
            if name in gr.QUIRK_CASES:
                assert nt.max() == int(cs["nconvlev"]) + 1 == int(cs["grid"][2]) - 1 and (nt == nt.max()).sum() >= 10, (name, kind, nt.max())
            else:
                assert nt.max() <= int(cs["nconvlev"]), (name, kind, nt.max())
            assert not rec["pconv"][:, -1].any(), (name, kind, "pconv(nuvz) is not zero in this build")
            assert not rec["fmassfrac"][lc == 0].any()
            snd = gr.soundings(cs, kind, cols, 0)
            for k in gr.SND_KEYS:
                assert np.array_equal(snd[k].astype(np.float64), rec[k]), f"{name} {kind}: the restatement differs from the reference in {k}"
            out = {k: v.astype(store) for k, v in rec.items() if k.startswith(("ztra1_", "cbaseflux_")) or k in gr.SND_KEYS + ("cbnew",)}
            out.update(cols=cols, lconv=lc, nconvtop=nt, exit=ex, fm_cols=np.flatnonzero(lc == 1).astype(np.int32),
                       fmassfrac=rec["fmassfrac"][lc == 1].astype(store), ncalls=np.int32(len(cs["itimes"])))
            for k, v in out.items():
                if v.dtype == np.float32:
                    assert np.array_equal(v.astype(np.float64), rec["fmassfrac"][lc == 1] if k == "fmassfrac" else rec[k]), (name, kind, k)
            todo[(name, kind)] = out
    for (name, kind), rec in todo.items():               # the condition of the device tests' bounds
        ref = gr.reference(name, kind, gold=rec)
        assert ref["noflip"], f"{name} {kind}: a libm perturbation flips a column: change the synthetic case"
        assert np.array_equal(ref["lconv"][0], rec["lconv"]) and np.array_equal(ref["nconvtop"][0], rec["nconvtop"]), (name, kind)
        print(f"{name} {kind}: noflip holds; largest |d fmassfrac|, |d uvzlev| under perturbation: {ref['dev_fm'].max():.3e}, {ref['dev_uvz'].max():.3e}")
    for (name, kind), rec in todo.items():               # nothing is written unless every case passed
        path = os.path.join(HERE, f"cvg_{name}_{kind}.npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print("wrote", os.path.basename(path), size, "bytes")


if __name__ == "__main__":
    main()
