"""Regenerates tests/golden/vtgfs_<case>_<kind>.npz: what the reference's own verttransform_gfs leaves in com_mod after each
of the three calls of a test case (tests/verttransform_gfs_ref.py: CASES, PHASES -- slot 1 with init, slot 2, slot 1 again).

The unmodified reference sources par_mod, com_mod, cmapf_mod, verttransform_gfs, ew and qvsat are compiled where they lie with
flang (-cpp -O2 -mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver tests/golden/ref_vg_driver.f90
into a build directory outside git (a temporary one unless --build-dir is given).  The routine keeps uvwzlev, an automatic
array of the full par_mod size (36 MB in r4, 72 MB in r8), on the stack, so the binary runs with the stack limit raised.
Nothing of the reference is copied; the fixtures hold outputs only (the tests regenerate the synthetic inputs bit for bit).

Before anything is written the script asserts, from the record of the restatement on the same inputs, the conditions the
tests rely on (verttransform_gfs_ref.check_conditions), and that the restatement equals the reference outside the mask.

What a fixture holds.  Three calls of eleven arrays do not fit the size limit of a committed file at the shapes of the cases
(`terrain`: 0.67 million values), so a fixture holds
  sha_<call>_<field>   the SHA-256 of the reference's array, every field of every call (ww with the masked cells set to zero,
                       uupol / vvpol on the cap rows): the bit-for-bit comparison of the CPU tests
  <field>_<call>       the arrays themselves as far as they fit: all of them for `cap`; for `flat` and `terrain` ww of every
                       call (the field with the history) and every field of the third call at the z levels LEVELS_KEPT
  height, nmixz
r4 values are exact in float32 and are stored so.

    python tests/golden/make_vtgfs_golden.py            # writes the six fixtures
    python tests/golden/make_vtgfs_golden.py --time     # the reference's seconds per 361 x 181 x 34 field, one core
"""
import argparse
import hashlib
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
OUT3 = ("uu", "vv", "ww", "tt", "qv", "pv", "rho", "drhodz", "pplev", "uupol", "vvpol")     # the driver's order
SOURCES = ("par_mod", "com_mod", "cmapf_mod", "verttransform_gfs", "ew", "qvsat")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """vgref_<kind> in build_dir/<kind> (an existing binary newer than the driver is kept)"""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"vgref_{kind}")
    drv = os.path.join(HERE, "ref_vg_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_vg_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_vg_driver.o"] + [s + ".o" for s in SOURCES[::-1]] + ["-o", exe], cwd=d)
    return exe


def _raise_stack():
    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def run(exe, calls, workdir, reps=0):
    """calls = [(slot, gfs_levels dict)]: one run of the driver, the calls sharing com_mod.  Returns one dict of float64
    arrays [nz][ny][nx] (+ height, nmixz) per call (and, with reps, the seconds per call the driver printed)."""
    m0 = calls[0][1]
    nx, ny, nz = (int(v) for v in m0["grid"])
    fin, fout = os.path.join(workdir, "vg_in.bin"), os.path.join(workdir, "vg_out.bin")
    with open(fin, "wb") as f:
        np.array([nx, ny, nz] + [int(v) for v in m0["globalflags"]] + [len(calls)], np.int32).tofile(f)
        np.asarray(m0["geom"], np.float64).tofile(f)
        for k in ("akz", "bkz", "aknew", "bknew"):
            np.ascontiguousarray(m0[k], np.float64).tofile(f)
        for slot, m in calls:
            np.array([slot], np.int32).tofile(f)
            for k in ("ps", "tt2", "td2", "tth", "qvh", "uuh", "vvh", "pvh", "wwh"):
                np.ascontiguousarray(m[k], np.float64).tofile(f)
    out = subprocess.check_output([exe, fin, fout] + ([str(reps)] if reps else []), text=True, preexec_fn=_raise_stack)
    res = []
    with open(fout, "rb") as f:
        for _ in calls:
            r = {"height": np.fromfile(f, np.float64, nz), "nmixz": int(np.fromfile(f, np.int32, 1)[0])}
            for k in OUT3:
                r[k] = np.fromfile(f, np.float64, nx * ny * nz).reshape(nz, ny, nx)
            res.append(r)
    if reps:
        return res, float(out.split()[-1])
    return res


def run_case(kw, phases, kind, build_dir):
    from flexpart_amd import synthetic as syn
    exe = build(kind, build_dir)
    return run(exe, [(slot, syn.gfs_levels(**kw, phase=ph)) for slot, ph in zip((1, 2, 1), phases)], build_dir)


LEVELS_KEPT = (0, 1, 2, -3, -2, -1)       # 0-based z levels of the third call's arrays kept for `flat` and `terrain`


def digest(a, store):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a.astype(store)).tobytes()).digest(), np.uint8)


def comparable(field, a, mask, rows):
    """The part of a reference array the tests compare: ww with the masked cells zeroed, uupol / vvpol on the cap rows."""
    if field == "ww":
        return np.where(mask, 0.0, a)
    if field in ("uupol", "vvpol"):
        return a[:, rows, :]
    return a


def fixture(case, kw, kind, refs, outs):
    import verttransform_gfs_ref as vr
    from flexpart_amd import synthetic as syn
    store = np.float32 if kind == "r4" else np.float64
    rows = vr.polar_rows(syn.gfs_levels(**kw))
    rec = {"height": refs[0]["height"], "nmixz": np.int32(refs[0]["nmixz"])}
    for n, (ref, (f, _)) in enumerate(zip(refs, outs)):
        mask = np.isnan(f["ww"])
        for k in OUT3:
            if k in ("uupol", "vvpol") and not rows.any():
                continue
            a = comparable(k, ref[k], mask, rows)
            rec[f"sha_{n}_{k}"] = digest(a, store)
            if case == "cap" or k == "ww":
                rec[f"{k}_{n}"] = a.astype(store)
            elif n == 2:
                rec[f"{k}_{n}"] = a[list(LEVELS_KEPT)].astype(store)
    return rec


def main():
    import verttransform_gfs_ref as vr
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="vgref_")
    if a.time:
        m = syn.gfs_levels(361, 181, 34, global_grid=True, polar=True, terrain=51000.0)
        for kind in ("r4", "r8"):
            exe = build(kind, bd)
            secs = [run(exe, [(1, m)], bd, reps=a.reps)[1] for _ in range(3)]
            print(f"{kind}: verttransform_gfs over 361 x 181 x 34, one core: {min(secs):.4f} s per wind field (three runs of {a.reps} calls: "
                  + ", ".join(f"{s:.4f}" for s in secs) + ")")
        return
    todo = []
    for case, kw in vr.CASES.items():
        for kind in ("r4", "r8"):
            outs = vr.run_case(kw, vr.PHASES, kind, vr.case_polemaps(kw, kind))
            vr.check_conditions(case, kw, outs)
            refs = run_case(kw, vr.PHASES, kind, bd)
            rows = vr.polar_rows(syn.gfs_levels(**kw))
            for n, (ref, (f, _)) in enumerate(zip(refs, outs)):
                mask = np.isnan(f["ww"])
                assert np.array_equal(ref["height"], f["height"]), (case, kind, n, "height")
                # :126-131 sets nmixz only if a z level lies above hmixmax (`cap` has none: com_mod's nmixz stays unset, the
                # restatement and the engine say nz)
                assert ref["nmixz"] == f["nmixz"] or not (ref["height"] > 4500.0).any(), (case, kind, n, "nmixz")
                for k in OUT3:
                    if k in ("uupol", "vvpol") and not rows.any():
                        continue
                    assert np.array_equal(comparable(k, ref[k], mask, rows), comparable(k, f[k], mask, rows)), \
                        f"{case} {kind} call {n}: the restatement differs from the reference in {k}"
            todo.append((case, kind, fixture(case, kw, kind, refs, outs)))
    for case, kind, rec in todo:               # nothing is written unless every case passed
        path = os.path.join(HERE, f"vtgfs_{case}_{kind}.npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print("wrote", os.path.basename(path), size, "bytes")


if __name__ == "__main__":
    main()
