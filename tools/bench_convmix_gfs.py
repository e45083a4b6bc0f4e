#!/usr/bin/env python3
"""Measures fpx_convmix on a GFS handle (fpx_conv_init_gfs) on one MI355X: 361 x 181 columns, 34 GFS levels, 1e7 particles,
both real kinds, next to the ECMWF call of tools/bench_convmix.py with the same number of levels on the same box (run as a
child process right after, so both figures come from one visit of one machine).

Prints ONE JSON line per kind: device time of one call (HIP events on the engine's stream; the median of --reps calls after one
warm-up call, every call from the same cbaseflux), the spread of the calls, how many columns carry a mass flux afterwards, and the
ECMWF figure.  --out DIR also writes convmix_gfs_<nx>x<ny>x<nz>_<kind>.json there.
    python tools/bench_convmix_gfs.py [--nx 361 --ny 181 --nz 34 --particles 1e7 --reps 5 --out profiles/r18]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a, real):
    from flexpart_amd import synthetic as syn
    from flexpart_amd.engine import Engine, RNG_PHILOX
    n = int(a.particles)
    cs = syn.convection_case_gfs(nx=a.nx, ny=a.ny, nz=a.nz, n=1000, ncalls=1)
    sc = syn.base_scenario(a.nx, a.ny, a.nz, global_grid=False, nsteps=1)
    eng = Engine(sc, compute_real_bytes=real, host_real_bytes=real, rng_mode=RNG_PHILOX, max_particles=n)
    eng.seed_particles(n, zmax=16000.0, itime0=0)
    eng.set_windtime(cs["memtime"], (1, 2))
    eng.conv_init_gfs(cs)
    eng.cbaseflux(cs["cbaseflux"])
    for slot in (1, 2):
        eng.upload_conv_gfs_fields(slot, *(np.asarray(cs[k])[slot - 1] for k in ("ps", "tt2", "td2", "tt", "qv", "pplev")))
    cb0 = eng.cbaseflux()
    eng.sort()                             # the order a run keeps the particles in
    ms, moved = [], 0
    for r in range(a.reps + 1):
        eng.cbaseflux(cb0)                 # every repetition does the same work
        t0 = time.perf_counter()
        moved = eng.convmix(0)
        wall = time.perf_counter() - t0
        if r:
            ms.append((eng.convmix_device_ms, wall * 1e3))
    cb1 = eng.cbaseflux()
    batches = eng.info("conv_batches")
    eng.close()
    dev = [m[0] for m in ms]
    return {"metric": "convmix on a GFS handle, one call", "value": float(np.median(dev)), "unit": "ms (device)", "higher_is_better": False,
            "dtype": "f64" if real == 8 else "f32", "data": "synthetic",
            "config": {"workload": f"{a.nx}x{a.ny} columns x {a.nz} GFS levels (nconvlev {int(cs['nconvlev'])}), {n:.0e} particles, every column holds "
                                   "particles, cell-sorted storage order, upload path", "reps": a.reps, "warmup_calls": 1},
            "device_ms_all_calls": dev, "device_ms_min": float(min(dev)), "device_ms_max": float(max(dev)),
            "wall_ms_whole_call": float(np.median([m[1] for m in ms])), "particles_moved": int(moved), "columns": a.nx * a.ny,
            "columns_with_mass_flux_after": int((cb1 > 0).sum()), "matrix_batches": int(batches), "us_per_column": float(np.median(dev)) * 1e3 / (a.nx * a.ny)}


def ecmwf_figure(a, real):
    """tools/bench_convmix.py with the same grid, level count, particles and kind, in a fresh process"""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_convmix.py"), "--nx", str(a.nx), "--ny", str(a.ny), "--nuvz", str(a.nz),
           "--particles", str(a.particles), "--reps", str(a.reps), "--real", str(real), "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        return {"error": out.stderr[-500:]}
    j = json.loads(out.stdout.strip().splitlines()[-1])
    return {"value": j["value"], "unit": j["unit"], "workload": j["config"]["workload"], "columns_with_mass_flux_after": j["columns_with_mass_flux_after"],
            "particles_moved": j["particles_moved"], "command": " ".join(os.path.relpath(c, ROOT) if os.path.isabs(c) and c.startswith(ROOT) else c for c in cmd[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=361)
    ap.add_argument("--ny", type=int, default=181)
    ap.add_argument("--nz", type=int, default=34)
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--real", type=int, default=0, choices=(0, 4, 8), help="0: both kinds")
    ap.add_argument("--no-ecmwf", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for real in ((4, 8) if a.real == 0 else (a.real,)):
        out = measure(a, real)
        if not a.no_ecmwf:
            out["ecmwf_call_same_box"] = ecmwf_figure(a, real)
        print(json.dumps(out), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"convmix_gfs_{a.nx}x{a.ny}x{a.nz}_r{real}.json"), "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
