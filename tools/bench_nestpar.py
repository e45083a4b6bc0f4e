#!/usr/bin/env python3
"""Time of fpx_calcpar_nest and fpx_getvdep_nest (calcpar_nests.f90:63-225 with getvdep_nests.f90) at the reference's own nest
size, 571 x 301 columns (par_mod_meteoswiss.f90:154): one JSON line per real kind with the device time of each kernel and
the time of each whole call (surfstrn, sshfn, excessoron resp. ssrn, lsprecn, convprecn, sdn up from pageable host arrays;
the model levels, ustarn, olin, psn, tt2n, td2n already on the device; the nest's gather packs written; no copy back).
The record is also written under profiles/.  --ref-r4 / --ref-r8: the reference's getvdep_nests on one core, seconds per
nest wind field, as `python tests/golden/make_getvdep_nests_golden.py --time` prints them where the reference can be built.
    python tools/bench_nestpar.py [--nxn 571 --nyn 301 --nz 138 --nspec 5 --reps 20 --out profiles/r13]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(a, real):
    import ctypes as C
    import time
    from flexpart_amd import synthetic as syn
    from flexpart_amd._lib import FpxCalcparIn, FpxGetvdepIn, check
    from flexpart_amd.engine import Engine
    m = syn.model_levels(nx=40, ny=24, nz=a.nz, global_grid=False)          # 1 degree, 20 W .. 19 E, 20 N .. 43 N
    dxn = 0.02
    assert (a.nxn - 1) * dxn <= 28.0 and (a.nyn - 1) * dxn <= 12.0, "the nest must fit the mother grid"
    n = syn.model_levels(nx=a.nxn, ny=a.nyn, nz=a.nz, global_grid=False, phase=3)
    for k in ("akz", "bkz", "aknew", "bknew"):
        n[k] = m[k].copy()
    n["geom"] = np.array([dxn, dxn, -15.0, 25.0])
    cin = syn.nest_calcpar_inputs(n)
    gin = syn.nest_getvdep_inputs(n)
    sc = dict(grid=m["grid"], geom=m["geom"], globalflags=m["globalflags"], nspec=a.nspec, npart=0)
    skip = ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep")
    sc.update({k: v for k, v in syn.base_scenario(8, 6, 5, nspec=a.nspec).items() if k not in sc and k not in skip})
    sc.update(drydep=1, drydepspec=np.ones(a.nspec, np.int32))
    eng = Engine(sc, compute_real_bytes=real, host_real_bytes=real)
    eng.init_nest((a.nxn, a.nyn), n["geom"])
    eng.getvdep_init(syn.getvdep_tables(40, 24, a.nspec))
    eng.getvdep_nest_init(1, syn.nest_getvdep_tables(n, a.nspec)["xlanduse"])
    eng.verttransform(1, m, None, init=True, want=())
    eng.verttransform(1, n, None, nest=1, want=())
    # the C calls alone, on host arrays that stay put (as com_mod's do), without the copies back
    rt = eng.hreal
    c = FpxCalcparIn()
    keep = {k: np.ascontiguousarray(np.asarray(cin[k]).astype(rt)) for k in ("surfstr", "sshf", "excessoro", "akm", "bkm")}
    for k, v in keep.items():
        setattr(c, k, v.ctypes.data)
    c.lsubgrid, c.device_vdep = int(cin["lsubgrid"]), 1
    g = FpxGetvdepIn()
    keepg = {k: np.ascontiguousarray(np.asarray(gin[k]).astype(rt)) for k in ("ssr", "lsprec", "convprec", "sd")}
    for k, v in keepg.items():
        setattr(g, k, v.ctypes.data)
    t = {k: [] for k in ("cp_dev", "cp_call", "gv_dev", "gv_call")}
    ms = C.c_double(0)
    for _ in range(a.reps + 3):
        t0 = time.perf_counter()
        check(eng.lib.fpx_calcpar_nest(eng.h, 1, 1, C.byref(c), None), "fpx_calcpar_nest")
        t["cp_call"].append((time.perf_counter() - t0) * 1e3)
        check(eng.lib.fpx_calcpar_time(eng.h, C.byref(ms)), "fpx_calcpar_time")
        t["cp_dev"].append(ms.value)
        t0 = time.perf_counter()
        check(eng.lib.fpx_getvdep_nest(eng.h, 1, 1, C.byref(g), None), "fpx_getvdep_nest")
        t["gv_call"].append((time.perf_counter() - t0) * 1e3)
        check(eng.lib.fpx_getvdep_time(eng.h, C.byref(ms)), "fpx_getvdep_time")
        t["gv_dev"].append(ms.value)
    eng.close()
    t = {k: v[3:] for k, v in t.items()}
    rec = {"metric": "calcpar_nest + getvdep_nest, one nest wind field", "value": float(np.median(t["cp_dev"]) + np.median(t["gv_dev"])),
           "unit": "ms (device, both kernels)", "higher_is_better": False, "dtype": "f64" if real == 8 else "f32", "data": "synthetic",
           "config": {"workload": f"{a.nxn}x{a.nyn} columns, {a.nz} levels, {a.nspec} species, 13 land-use classes, 11 diameter intervals", "reps": a.reps, "warmup": 3}}
    for k, v in t.items():
        rec[k + "_ms_median"] = float(np.median(v))
        rec[k + "_ms_min_max"] = [float(min(v)), float(max(v))]
    ref = a.ref_r8 if real == 8 else a.ref_r4
    if ref is not None:
        rec["reference_getvdep_nests_one_core_s"] = float(ref)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nxn", type=int, default=571)
    ap.add_argument("--nyn", type=int, default=301)
    ap.add_argument("--nz", type=int, default=138)
    ap.add_argument("--nspec", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ref-r4", type=float, default=None)
    ap.add_argument("--ref-r8", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for real in (4, 8):
        rec = one(a, real)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out, f"nestpar_{a.nxn}x{a.nyn}_{rec['dtype']}_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
