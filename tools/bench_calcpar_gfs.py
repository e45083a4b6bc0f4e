#!/usr/bin/env python3
"""Time of fpx_calcpar_gfs (the NCEP branch of calcpar on the device) at 361x181 and 721x361 with 34 levels, in both real
kinds, next to fpx_calcpar (the ECMWF branch) on a grid of the same size in the same run.  One JSON line per grid and kind,
also written to <out>/calcpar_gfs_<nx>x<ny>x<nz>_<kind>.json, with
  * kernel_ms: the device time of k_calcpar_gfs (fpx_calcpar_time);
  * call_ms: the wall time of the whole call -- surfstr, sshf, hmix, excessoro over PCIe (pageable host arrays), the kernel,
    the packing into the gather layout, hcell, and the five 2-D results copied back;
  * ecmwf_kernel_ms, ecmwf_call_ms: the same two numbers of fpx_calcpar after fpx_verttransform_ecmwf of as many columns
    and levels;
  * reference_s: the seconds the unmodified calcpar (NCEP branch, with the calcpv it calls) takes per 361x181x34 field on one
    core, as tests/golden/make_cpg_golden.py --time printed them where the reference builds (--ref-seconds r4=.. r8=..);
  * bytes_read: what the kernel reads by its own count (tth, qvh twice -- richardson and the tropopause --, uuh, vvh over the
    levels a column visits are not counted exactly: the whole of the four 3-D arrays once, the 2-D inputs), and the rate
    that gives.  At 65 000 columns the grid is about one wave per SIMD: the time is the latency of one column's dependent
    chain of log / pow calls, not bandwidth.
Nothing is asserted on these numbers.  Median of --reps calls after 3.
    python tools/bench_calcpar_gfs.py [--grids 361x181 721x361 --nz 34 --real 8 4 --reps 20 --out profiles/r17]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 3
DROP = ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "uupol", "vvpol", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep")


def engine(nx, ny, nz, rb):
    from flexpart_amd import synthetic as syn
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = syn.base_scenario(nx, ny, nz, nsteps=1)
    for k in DROP:
        sc.pop(k, None)
    return Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=RNG_PHILOX)


def measure(nx, ny, nz, rb, reps):
    from flexpart_amd import synthetic as syn
    m = syn.gfs_levels(nx, ny, nz, terrain=25000.0)
    cin = syn.calcpar_gfs_inputs(m)
    eng = engine(nx, ny, nz, rb)
    eng.verttransform_gfs(1, m, {}, init=True, want=())
    call, dev = [], []
    for _ in range(reps + WARMUP):
        r = eng.calcpar_gfs(1, cin)
        call.append(r["call_ms"]); dev.append(r["device_ms"])
    eng.close()
    me = syn.model_levels(nx=nx, ny=ny, nz=nz, polar=False)
    ce = syn.calcpar_inputs(me)
    eng = engine(nx, ny, nz, rb)
    eng.verttransform(1, me, None, init=True, want=())
    ecall, edev = [], []
    for _ in range(reps + WARMUP):
        t0 = time.perf_counter()
        r = eng.calcpar(1, ce)
        ecall.append((time.perf_counter() - t0) * 1e3); edev.append(r["device_ms"])
    eng.close()
    call, dev, ecall, edev = call[WARMUP:], dev[WARMUP:], ecall[WARMUP:], edev[WARMUP:]
    k = float(np.median(dev))
    read = (4 * nx * ny * nz + 7 * nx * ny) * rb
    return {"metric": "calcpar_gfs on the device, one wind field", "value": k, "unit": "ms (device, k_calcpar_gfs)", "higher_is_better": False,
            "dtype": "f64" if rb == 8 else "f32", "data": "synthetic",
            "config": {"workload": f"{nx}x{ny}x{nz} GFS pressure levels, terrain down to 770 hPa", "reps": reps, "warmup": WARMUP},
            "kernel_ms": k, "kernel_ms_min_max": [float(min(dev)), float(max(dev))],
            "call_ms": float(np.median(call)), "call_ms_min_max": [float(min(call)), float(max(call))],
            "ecmwf_kernel_ms": float(np.median(edev)), "ecmwf_call_ms": float(np.median(ecall)),
            "columns": nx * ny, "waves": (nx * ny + 63) // 64,
            "input_bytes_over_pcie": 4 * nx * ny * rb, "bytes_read": read, "read_GBps": read / k / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["361x181", "721x361"])
    ap.add_argument("--nz", type=int, default=34)
    ap.add_argument("--real", type=int, nargs="+", default=[8, 4], choices=(4, 8))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ref-seconds", nargs="*", default=[], help="r4=<s> r8=<s>: make_cpg_golden.py --time, 361x181x34, one core")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17"))
    a = ap.parse_args()
    ref = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in a.ref_seconds}
    os.makedirs(a.out, exist_ok=True)
    for g in a.grids:
        nx, ny = (int(v) for v in g.split("x"))
        for rb in a.real:
            kind = "r8" if rb == 8 else "r4"
            res = measure(nx, ny, a.nz, rb, a.reps)
            if kind in ref:
                res["reference_s"] = ref[kind]
                res["reference_workload"] = "361x181x34, one core, calcpar with its calcpv"
            print(json.dumps(res), flush=True)
            with open(os.path.join(a.out, f"calcpar_gfs_{nx}x{ny}x{a.nz}_{kind}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
