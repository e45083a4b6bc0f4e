"""Regenerates tests/golden/cpg_<case>_<kind>.npz -- what the reference's own calcpar leaves in ustar, wstar, oli, hmix and
tropopause of the slot after each of the three calls of a test case with metdata_format = GRIBFILE_CENTRE_NCEP
(tests/calcpar_gfs_ref.py: CASES, RUNS; slot 1, slot 2, slot 1 again with verttransform_gfs_ref.PHASES) -- and
tests/golden/cp_ecmwf_<kind>.npz, one call of the same routine with metdata_format = GRIBFILE_CENTRE_ECMWF on
synthetic.model_levels(nx=60, ny=40, nz=60) + calcpar_inputs.

The unmodified reference sources par_mod, com_mod, calcpar, obukhov, richardson, scalev, ew, qvsat, calcpv and the getvdep chain
(linked, never called: DRYDEP is false) are compiled where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind with
-fdefault-real-8) together with our stand-in for class_gribfile (class_gribfile_standin.f90: three integer parameters) and
our driver ref_cpg_driver.f90, into a build directory outside git (a temporary one unless --build-dir is given).  Nothing of
the reference is copied; the fixtures hold outputs only (the tests regenerate the synthetic inputs bit for bit).  Keys:
<field>_<call>_ls<lsubgrid> for the NCEP cases, <field> for ECMWF; r4 values are exact in float32 and are stored so.

Before anything is written the script asserts, from the record of the restatement on the same inputs, the conditions the
tests rely on (calcpar_gfs_ref.check_conditions), that the restatement equals the reference bit for bit, and that the shares
of fragile columns (margin below the reach of tests/test_calcpar.py) stay within what the GPU test allows.

    python tests/golden/make_cpg_golden.py            # writes the six fixtures
    python tests/golden/make_cpg_golden.py --time     # the reference's seconds per 361 x 181 x 34 field, one core
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
FIELDS = ("ustar", "wstar", "oli", "hmix", "tropopause")          # the driver's order
SOURCES = ("par_mod", "com_mod", "calcpar", "obukhov", "richardson", "scalev", "ew", "qvsat", "calcpv",
           "getvdep", "getrb", "getrc", "raerod", "psih", "partdep", "caldate")
NCEP, ECMWF = 1, 2
ECMWF_CASE = dict(nx=60, ny=40, nz=60)


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """cpgref_<kind> in build_dir/<kind> (an existing binary newer than the driver is kept)"""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"cpgref_{kind}")
    drv = os.path.join(HERE, "ref_cpg_driver.f90")
    standin = os.path.join(HERE, "class_gribfile_standin.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(drv), os.path.getmtime(standin)):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    for s in SOURCES[:2]:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
    subprocess.check_call([FC, "-c"] + flags + [standin, "-o", "class_gribfile.o"], cwd=d)
    for s in SOURCES[2:]:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_cpg_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_cpg_driver.o", "class_gribfile.o"] + [s + ".o" for s in SOURCES[::-1]] + ["-o", exe], cwd=d)
    return exe


def _raise_stack():
    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def write_input(path, calls, fmt, lsubgrid):
    """calls = [(slot, level dict, cin)]: the driver's input file (also read by tests/calcpar_gfs_host.cpp)"""
    m0, c0 = calls[0][1], calls[0][2]
    nx, ny, nz = (int(v) for v in m0["grid"])
    zero = np.zeros(nz)
    with open(path, "wb") as f:
        np.array([nx, ny, nz] + [int(v) for v in m0["globalflags"]] + [len(calls), fmt, lsubgrid], np.int32).tofile(f)
        np.asarray(m0["geom"], np.float64).tofile(f)
        for a in (m0["akz"], m0["bkz"], c0.get("akm", zero), c0.get("bkm", zero), c0["excessoro"]):
            np.ascontiguousarray(a, np.float64).tofile(f)
        for slot, m, c in calls:
            np.array([slot], np.int32).tofile(f)
            for a in (m["ps"], m["tt2"], m["td2"], c["surfstr"], c["sshf"], c.get("hmix", np.zeros((ny, nx))), m["tth"], m["qvh"], m["uuh"], m["vvh"]):
                np.ascontiguousarray(a, np.float64).tofile(f)


def read_output(path, ncalls, ny, nx):
    with open(path, "rb") as f:
        return [{k: np.fromfile(f, np.float64, nx * ny).reshape(ny, nx) for k in FIELDS} for _ in range(ncalls)]


def run(exe, calls, fmt, lsubgrid, workdir, reps=0):
    """One run of the driver, the calls sharing com_mod.  Returns one dict of float64 [ny][nx] arrays per call (and, with
    reps, the seconds per call the driver printed)."""
    nx, ny, _ = (int(v) for v in calls[0][1]["grid"])
    fin, fout = os.path.join(workdir, "cpg_in.bin"), os.path.join(workdir, "cpg_out.bin")
    write_input(fin, calls, fmt, lsubgrid)
    out = subprocess.check_output([exe, fin, fout] + ([str(reps)] if reps else []), text=True, preexec_fn=_raise_stack)
    res = read_output(fout, len(calls), ny, nx)
    if reps:
        return res, float(out.split()[-1])
    return res


def ncep_calls(case, lsubgrid):
    import calcpar_gfs_ref as cr
    return [cr.case_inputs(case, lsubgrid, n) for n in range(3)]


def ecmwf_call():
    from flexpart_amd import synthetic as syn
    m = syn.model_levels(**ECMWF_CASE)
    return [(1, m, syn.calcpar_inputs(m))]


def main():
    import calcpar_gfs_ref as cr
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="cpgref_")
    if a.time:
        m = syn.gfs_levels(361, 181, 34, terrain=25000.0)
        c = syn.calcpar_gfs_inputs(m)
        for kind in ("r4", "r8"):
            exe = build(kind, bd)
            secs = [run(exe, [(1, m, c)], NCEP, 1, bd, reps=a.reps)[1] for _ in range(3)]
            print(f"{kind}: calcpar (NCEP branch, with its calcpv) over 361 x 181 x 34, one core: {min(secs):.4f} s per wind field "
                  f"(three runs of {a.reps} calls: " + ", ".join(f"{s:.4f}" for s in secs) + ")")
        return
    todo = {}
    for kind in ("r4", "r8"):
        store = np.float32 if kind == "r4" else np.float64
        exe = build(kind, bd)
        unfired = 0
        for case, ls in cr.RUNS:
            calls = ncep_calls(case, ls)
            outs = cr.run_case(case, ls, kind)
            unfired += cr.check_conditions(case, outs, [c for _, _, c in calls])
            refs = run(exe, calls, NCEP, ls, bd)
            rec = todo.setdefault((f"cpg_{case}", kind), {})
            for n, (ref, (f, r)) in enumerate(zip(refs, outs)):
                for k in FIELDS:
                    assert np.array_equal(ref[k], f[k]), \
                        f"{case} ls={ls} {kind} call {n}: the restatement differs from the reference in {k} ({int((ref[k] != f[k]).sum())} columns)"
                    rec[f"{k}_{n}_ls{ls}"] = ref[k].astype(store)
                share = float(cr.fragile(r, kind).mean())
                assert share <= cr.FRAGILE_SHARE[kind], f"{case} ls={ls} {kind} call {n}: fragile share {share:.4f}"
                print(f"{case} ls={ls} {kind} call {n}: fragile share {share:.4f}, smallest margin {r['margin'].min():.3e}, "
                      f"tropopause not fired in {int((~r['tropo_fired']).sum())} columns")
        if unfired == 0:
            print(f"{kind}: NO column of any call exercises a tropopause criterion that does not fire")
        todo[("cp_ecmwf", kind)] = {k: v.astype(store) for k, v in run(exe, ecmwf_call(), ECMWF, 1, bd)[0].items()}
    for (name, kind), rec in todo.items():               # nothing is written unless every case passed
        path = os.path.join(HERE, f"{name}_{kind}.npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print("wrote", os.path.basename(path), size, "bytes")


if __name__ == "__main__":
    main()
