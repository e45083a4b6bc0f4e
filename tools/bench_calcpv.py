#!/usr/bin/env python3
"""Time of calcpv on the device (fpx_verttransform_ecmwf with pvh = NULL) at the BASELINE grid, and of what it replaces:
the PCIe time of one model-level array.  One JSON line per real kind with
  * the device time of the PV kernels (k_theta + k_pv + k_pole, HIP events);
  * the wall time of the whole fpx_verttransform_ecmwf call with device_pv on and off, from pageable host arrays and from
    arrays registered for DMA (pin_host); the difference off - on is the copy of pvh the kernels have to beat.
Median of --reps calls after 3.
    python tools/bench_calcpv.py [--nx 361 --ny 181 --nz 138 --real 8 4 --reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 3


def measure(a, rb):
    from flexpart_amd import synthetic as syn
    from flexpart_amd.engine import Engine, RNG_PHILOX
    nx, ny, nz = a.nx, a.ny, a.nz
    m = syn.model_levels(nx=nx, ny=ny, nz=nz, global_grid=True, polar=True)
    sc = syn.base_scenario(nx, ny, nz, polar=True, nsteps=1)
    sfc = {k: sc[k][0] for k in ("hmix", "ustar", "wstar", "oli", "tropopause")}
    for k in ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "uupol", "vvpol", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep"):
        sc.pop(k, None)
    eng = Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=RNG_PHILOX)
    eng.verttransform(1, m, sfc, init=True, want=())          # allocations, z levels
    res = {}
    for pinned in (False, True):
        for on in (True, False):
            # pinned: host arrays that stay put (the Fortran host's static com_mod arrays), registered once; the first call
            # registers them and is part of the warm-up.  The mirror's own marshalling is outside call_ms.
            held = {} if pinned else None
            call, dev, pv = [], [], []
            for _ in range(a.reps + WARMUP):
                r = eng.verttransform(2, m, sfc, want=(), host_arrays=held, device_pv=on)
                call.append(r["call_ms"]); dev.append(r["device_ms"]); pv.append(r["calcpv_ms"])
            call, dev, pv = call[WARMUP:], dev[WARMUP:], pv[WARMUP:]
            res[("pinned" if pinned else "pageable", "on" if on else "off")] = dict(
                call_ms=float(np.median(call)), call_ms_min_max=[float(min(call)), float(max(call))],
                transform_ms=float(np.median(dev)), calcpv_ms=float(np.median(pv)), calcpv_ms_min_max=[float(min(pv)), float(max(pv))])
    eng.close()
    pvk = res[("pinned", "on")]["calcpv_ms"]
    copy_pinned = res[("pinned", "off")]["call_ms"] - res[("pinned", "on")]["call_ms"] + pvk
    copy_pageable = res[("pageable", "off")]["call_ms"] - res[("pageable", "on")]["call_ms"] + res[("pageable", "on")]["calcpv_ms"]
    return {"metric": "calcpv on the device, one wind field", "value": pvk, "unit": "ms (device, k_theta + k_pv + k_pole)", "higher_is_better": False,
            "dtype": "f64" if rb == 8 else "f32", "data": "synthetic",
            "config": {"workload": f"{nx}x{ny}x{nz} model levels, xglobal + both poles", "reps": a.reps, "warmup": WARMUP},
            "pvh_bytes": nx * ny * nz * rb,
            "whole_call_ms": {f"{h}, device_pv {o}": v for (h, o), v in res.items()},
            # whole call (off) - whole call (on) = copy of pvh - PV kernels, so the copy alone is the difference plus the kernels
            "pvh_copy_ms_implied": {"pinned": copy_pinned, "pageable": copy_pageable},
            "saved_per_call_ms": {"pinned": res[("pinned", "off")]["call_ms"] - res[("pinned", "on")]["call_ms"],
                                  "pageable": res[("pageable", "off")]["call_ms"] - res[("pageable", "on")]["call_ms"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=361)
    ap.add_argument("--ny", type=int, default=181)
    ap.add_argument("--nz", type=int, default=138)
    ap.add_argument("--real", type=int, nargs="+", default=[8, 4], choices=(4, 8))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for rb in a.real:
        print(json.dumps(measure(a, rb)), flush=True)


if __name__ == "__main__":
    main()
