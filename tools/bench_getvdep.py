#!/usr/bin/env python3
"""Time of fpx_getvdep (the dry-deposition velocities of calcpar.f90:171-189) at the BASELINE grid: one JSON line with the
device time of the kernel and the time of the whole call (four 2-D fields up; ustar, oli, ps, tt2, td2 already on the
device from fpx_verttransform_ecmwf and fpx_calcpar; the gather pack written; no copy back).
    python tools/bench_getvdep.py [--nx 361 --ny 181 --nz 138 --nspec 5 --real 8]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=361)
    ap.add_argument("--ny", type=int, default=181)
    ap.add_argument("--nz", type=int, default=138)
    ap.add_argument("--nspec", type=int, default=5)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import ctypes as C
    import time
    from flexpart_amd import synthetic as syn
    from flexpart_amd._lib import FpxGetvdepIn, check
    from flexpart_amd.engine import Engine
    m = syn.model_levels(nx=a.nx, ny=a.ny, nz=a.nz, polar=False)
    cin = syn.calcpar_inputs(m)
    gin = syn.getvdep_inputs(m)
    sc = dict(grid=m["grid"], geom=m["geom"], globalflags=m["globalflags"], nspec=a.nspec, npart=0)
    skip = ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep")
    sc.update({k: v for k, v in syn.base_scenario(8, 6, 5, nspec=a.nspec).items() if k not in sc and k not in skip})
    sc.update(drydep=1, drydepspec=np.ones(a.nspec, np.int32))
    eng = Engine(sc, compute_real_bytes=a.real, host_real_bytes=a.real)
    eng.getvdep_init(syn.getvdep_tables(a.nx, a.ny, a.nspec))
    eng.verttransform(1, m, None, init=True, want=())
    eng.calcpar(1, cin, device_vdep=True)
    # the C call alone, on host arrays that stay put (as com_mod's do), without the copy back
    g = FpxGetvdepIn()
    keep = {k: np.ascontiguousarray(np.asarray(gin[k]).astype(eng.hreal)) for k in ("ssr", "lsprec", "convprec", "sd")}
    for k, v in keep.items():
        setattr(g, k, v.ctypes.data)
    dev, call = [], []
    for _ in range(a.reps + 3):
        t0 = time.perf_counter()
        check(eng.lib.fpx_getvdep(eng.h, 1, C.byref(g), None), "fpx_getvdep")
        call.append((time.perf_counter() - t0) * 1e3)
        ms = C.c_double(0)
        check(eng.lib.fpx_getvdep_time(eng.h, C.byref(ms)), "fpx_getvdep_time")
        dev.append(ms.value)
    eng.close()
    dev, call = dev[3:], call[3:]
    print(json.dumps({"metric": "getvdep, one wind field", "value": float(np.median(dev)), "unit": "ms (device)", "higher_is_better": False,
                      "call_ms_median": float(np.median(call)), "device_ms_min_max": [float(min(dev)), float(max(dev))],
                      "call_ms_min_max": [float(min(call)), float(max(call))],
                      "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic",
                      "config": {"workload": f"{a.nx}x{a.ny} columns, {a.nspec} species, 13 land-use classes, 11 diameter intervals", "reps": a.reps, "warmup": 3}}), flush=True)


if __name__ == "__main__":
    main()
