#!/usr/bin/env python3
"""Time of fpx_verttransform_gfs (NCEP GFS pressure levels -> z levels on the device) at 361x181 and 721x361 with 34 levels,
in both real kinds.  One JSON line per grid and kind, also written to <out>/vtgfs_<nx>x<ny>x<nz>_<kind>.json, with
  * kernel_ms: the device time of the transform kernels (fpx_verttransform_time: k_vg_levels + k_vg_column + the caps);
  * call_ms: the wall time of the whole call -- the copy of the nine input arrays over PCIe (pageable host arrays), the
    kernels, the repacking into the gather layout; no z-level array is copied back;
  * algorithmic_bytes: what any implementation has to move (six 3-D inputs read, nine 3-D outputs written), plan_bytes: what
    the two-kernel plan moves through HBM by its own count (uvwzlev written once and read back once, tth and qvh read by both
    kernels; neighbour columns' uvwzlev and the re-reads for pinmconv are expected from L2 and not counted -- not a counter
    measurement), and the rates both give against kernel_ms.
Median of --reps calls after 3.
    python tools/bench_verttransform_gfs.py [--grids 361x181 721x361 --nz 34 --real 8 4 --reps 20 --out profiles/r15]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 3


def measure(nx, ny, nz, rb, reps):
    from flexpart_amd import synthetic as syn
    from flexpart_amd.engine import Engine, RNG_PHILOX
    ms = [syn.gfs_levels(nx, ny, nz, global_grid=True, polar=True, phase=p, terrain=51000.0) for p in (0, 5)]
    sc = syn.base_scenario(nx, ny, nz, polar=True, nsteps=1)
    sfc = {k: sc[k][0] for k in ("hmix", "ustar", "wstar", "oli", "tropopause")}
    for k in ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "uupol", "vvpol", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep"):
        sc.pop(k, None)
    eng = Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=RNG_PHILOX)
    eng.verttransform_gfs(1, ms[0], sfc, init=True, want=())          # allocations, z levels
    call, dev = [], []
    for n in range(reps + WARMUP):
        r = eng.verttransform_gfs(1 + n % 2, ms[n % 2], sfc, want=())
        call.append(r["call_ms"]); dev.append(r["device_ms"])
    eng.close()
    call, dev = call[WARMUP:], dev[WARMUP:]
    n3 = nx * ny * nz * rb
    algo, plan = (6 + 9) * n3, (6 + 2 + 1 + 1 + 9) * n3
    k = float(np.median(dev))
    return {"metric": "verttransform_gfs on the device, one wind field", "value": k, "unit": "ms (device, transform kernels)", "higher_is_better": False,
            "dtype": "f64" if rb == 8 else "f32", "data": "synthetic",
            "config": {"workload": f"{nx}x{ny}x{nz} GFS pressure levels, both poles, terrain down to 510 hPa", "reps": reps, "warmup": WARMUP},
            "kernel_ms": k, "kernel_ms_min_max": [float(min(dev)), float(max(dev))],
            "call_ms": float(np.median(call)), "call_ms_min_max": [float(min(call)), float(max(call))],
            "input_bytes_over_pcie": (6 * nx * ny * nz + 3 * nx * ny) * rb,
            "algorithmic_bytes": algo, "plan_bytes": plan,
            "algorithmic_GBps": algo / k / 1e6, "plan_GBps": plan / k / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["361x181", "721x361"])
    ap.add_argument("--nz", type=int, default=34)
    ap.add_argument("--real", type=int, nargs="+", default=[8, 4], choices=(4, 8))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for g in a.grids:
        nx, ny = (int(v) for v in g.split("x"))
        for rb in a.real:
            res = measure(nx, ny, a.nz, rb, a.reps)
            print(json.dumps(res), flush=True)
            with open(os.path.join(a.out, f"vtgfs_{nx}x{ny}x{a.nz}_{'r8' if rb == 8 else 'r4'}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
