"""Regenerates tests/golden/oh_r4.npz and oh_r8.npz: OH_hourly and memOHtime after every gethourlyOH and xmass1 after every
ohreaction that the reference's own routines produce for flexpart_amd.synthetic.oh_case(), both run directions.

The reference sources (par_mod_meteoswiss -- the reference's own variant of par_mod with maxnests = 1 and maxspec = 5; the
shipped par_mod has no room for a nest or a second species --, com_mod, oh_mod, caldate, zenithangle, photo_O1D, gethourlyOH,
ohreaction) are compiled where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver
tests/golden/ref_oh_driver.f90 into a build directory outside git (a temporary one unless --build-dir is given).  Nothing of
the reference is copied or written anywhere.  The fixtures hold results only; the tests regenerate the inputs bit for bit.

Before anything is written the maker asserts, from the record of the restatement tests/ohreaction_ref.py, that the case
decides nothing by a hair (check_conditions): a fixture is only as good as the margins of its inputs.

    python tests/golden/make_ohreaction_golden.py [--time N]

--time N: also times one ohreaction of the reference over N storage spaces on one core (the case's particles repeated)."""
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
SOURCES = ("par_mod_meteoswiss", "com_mod", "oh_mod", "caldate", "zenithangle", "photo_O1D", "gethourlyOH", "ohreaction")
KINDS = ("r4", "r8")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """ohref_<kind> in build_dir (built once: an existing binary newer than the driver is kept)."""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"ohref_{kind}")
    drv = os.path.join(HERE, "ref_oh_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    objs = []
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_oh_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_oh_driver.o"] + objs[::-1] + ["-o", exe], cwd=d)
    return exe


def write_input(c, kind, path):
    from flexpart_amd import synthetic as syn
    nx, ny, nz = (int(v) for v in c["grid"])
    nxo, nyo, nzo = (int(v) for v in c["ohgrid"])
    n = int(c["npart"])
    with open(path, "wb") as f:
        np.array([nx, ny, nz, n, nxo, nyo, nzo, c["nspec"], c["ldirect"], len(c["calls"]), c["nest"][0], c["nest"][1]], np.int32).tofile(f)
        np.array(list(c["geom"]) + [c["bdate"]] + list(c["nestgeom"]), np.float64).tofile(f)
        for k in ("height", "lonOH", "latOH", "altOH", "lonjr", "latjr", "jrate_average", "OH_field"):
            np.ascontiguousarray(c[k], np.float64).tofile(f)                 # C order [m][kz][jy][ix] = Fortran (ix,jy,kz,m)
        for m in range(2):
            np.ascontiguousarray(c["tt"][m], np.float64).tofile(f)
        for k in ("ohcconst", "ohdconst", "ohnconst", "xtra1", "ytra1", "ztra1"):
            np.asarray(c[k], np.float64).tofile(f)
        syn.oh_masses(c, kind).astype(np.float64).tofile(f)                  # [nspec][n] = Fortran (n,nspec)
        for call in c["calls"]:
            if call[0] == "hourly":
                np.array([0, call[1], 0, 0, 0, 1, 2], np.int32).tofile(f)
            else:
                _, itime, lts, mt, mi = call
                np.array([1, itime, lts, mt[0], mt[1], mi[0], mi[1]], np.int32).tofile(f)


def run(exe, c, kind, workdir, ntime=0):
    """One pass of the driver: per call a dict like ohreaction_ref.run_case gives (OH_hourly, memOHtime | xmass1), float64."""
    os.makedirs(workdir, exist_ok=True)
    fin, fout = os.path.join(workdir, "oh_in.bin"), os.path.join(workdir, "oh_out.bin")
    write_input(c, kind, fin)
    out = subprocess.check_output([exe, fin, fout] + ([str(int(ntime))] if ntime else []), text=True)
    if ntime:
        print(f"[{kind}] {out.strip()}")
    nxo, nyo, nzo = (int(v) for v in c["ohgrid"])
    n, nspec = int(c["npart"]), int(c["nspec"])
    res = []
    with open(fout, "rb") as f:
        for call in c["calls"]:
            if call[0] == "hourly":
                mt = np.fromfile(f, np.float64, 2)
                res.append(dict(kind="hourly", memOHtime=mt, OH_hourly=np.fromfile(f, np.float64, 2 * nzo * nyo * nxo).reshape(2, nzo, nyo, nxo)))
            else:
                res.append(dict(kind="react", xmass1=np.fromfile(f, np.float64, nspec * n).reshape(nspec, n)))
        assert f.read() == b""
    return res


def check_conditions(c, kind):
    """What the case must offer, from the restatement's record (the CPU tests assert the same): raises AssertionError."""
    import ohreaction_ref as oref
    from flexpart_amd import synthetic as syn
    res, o = oref.run_case(c, kind, syn.oh_masses(c, kind))
    assert [r["branch"] for r in res if r["kind"] == "hourly"] == [oref.BR_INIT, oref.BR_ADVANCE, oref.BR_NONE]
    assert o.months[0] != o.months[1]
    n = int(c["npart"])
    dead = np.asarray(c["itra1"]) == oref.DEAD
    assert 0 < dead.sum() <= 0.1 * n
    reacts = [r for r in res if r["kind"] == "react"]
    assert [r["rec"]["n"] for r in reacts] == [1, 2] and reacts[1]["memind"] == (2, 1)
    tt = np.asarray(c["tt"])
    for ax in range(4):                                                       # neighbours in slot, z, y, x differ by >= 8 K
        assert np.abs(np.diff(tt, axis=ax)).min() >= 8.0
    for r in reacts:
        rec = r["rec"]
        live = rec["live"]
        assert not rec["nolevel"].any() and not rec["ties"].any() and not rec["outside"].any()
        assert rec["ngrid"][live].sum() >= 0.3 * live.sum() and (rec["ngrid"] == 0)[live].sum() >= 0.3 * live.sum()
        assert rec["wrapped"][live].any() and (~rec["wrapped"])[live].any()
        assert rec["react"][live].any() and (~rec["react"])[live].any()       # oh_average > tiny: both outcomes
        assert (rec["oh"][~rec["react"]] == 0.0).all()
        assert len(set(rec["ohz"][live])) >= 3 and len(set(rec["ohx"][live])) >= 4 and len(set(rec["ohy"][live])) >= 4
        z = rec["zeroed"][:, live]
        assert z.any() and (~z[[0, 2]][:, rec["react"][live]]).any()          # restmass > tiny: both outcomes
        # the blended OH of neighbouring lit cells differs by far more than any rounding
        b = r["blend"].astype(np.float64)
        for ax in range(3):
            lo, hi = np.take(b, range(b.shape[ax] - 1), axis=ax), np.take(b, range(1, b.shape[ax]), axis=ax)
            both = (lo > 0) & (hi > 0)
            assert (np.abs(hi - lo)[both] > 1.0e-3 * np.maximum(hi, lo)[both]).all()
    r0 = reacts[0]["rec"]
    hot, tiny_p = int(c["hot_particle"]), int(c["tiny_particle"])
    lt = abs(reacts[0]["ltsample"])
    assert (r0["rates"][[0, 2], hot] * lt > 800.0).all() and (reacts[0]["xmass1"][[0, 2], hot] == 0).all()
    assert 0.02 < np.exp(-r0["rates"][0, tiny_p] * lt) < 0.2 and reacts[0]["xmass1"][0, tiny_p] == 0 and reacts[0]["xmass1"][2, tiny_p] > 0
    jr_le0 = sum(int((np.asarray(c["jrate_average"])[m - 1][o.jjy[:, None], o.ijx[None, :]] <= 0).sum()) for m in o.months)
    assert jr_le0 >= 2
    assert (o.sza1 >= 90).any() and (o.sza1 < 90).any()
    return res


def main():
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--time", type=int, default=0)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="ohref_")
    for kind in KINDS:
        exe = build(kind, bd)
        rec = {}
        for ld in syn.OH_DIRECTIONS:
            c = syn.oh_case(ld)
            check_conditions(c, kind)
            rt = np.float32 if kind == "r4" else np.float64
            tag = "f" if ld == 1 else "b"
            for ic, r in enumerate(run(exe, c, kind, os.path.join(bd, kind), ntime=a.time if ld == 1 else 0)):
                if r["kind"] == "hourly":
                    rec[f"{tag}_OH_hourly_{ic}"] = r["OH_hourly"].astype(rt)
                    rec[f"{tag}_memOHtime_{ic}"] = r["memOHtime"].astype(rt)
                else:
                    rec[f"{tag}_xmass1_{ic}"] = r["xmass1"].astype(rt)
        out = os.path.join(HERE, f"oh_{kind}.npz")
        np.savez_compressed(out, **rec)
        print("wrote", os.path.basename(out), os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
