#!/usr/bin/env python3
"""Measures fpx_plumetraj (plume trajectories and their clustering) on one MI355X: 361x181x138 met grid,
one seeded cloud, in two configurations -- (i) all particles in one release point, (ii) spread over 100 release points --
warmed up, by the call's own device events (fpx_plumetraj_time; the passes of the k-means loop by
fpx_get_info("plumetraj_sweep_us")).  In the same run it times fpx_download_particles of xtra1, ytra1, ztra1, itra1 and
npoint: the traffic the call replaces (the reference's host loop would follow it).
Prints ONE JSON line and, with --out, writes it to that file.
    python tools/bench_plumetraj.py [--particles 1e7 --real 8 --calls 3 --out profiles/r12/plumetraj_1e7_f64.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scenario():
    from flexpart_amd import synthetic as syn
    sc = syn.base_scenario(ctl=5.0, ifine=4, cblflag=0, nsteps=1)
    sc["npart"] = 1
    syn.add_partoutput_fields(sc, itime=0, dead_every=0)
    sc["pv"] = sc["pv"] * 2.0e6
    for k in ("npart", "itra1", "npoint"):
        del sc[k]
    return sc


def positions(eng, n):
    """fpx_download_particles of the five arrays plumetraj reads: (arrays, best wall ms of three)."""
    from flexpart_amd._lib import FpxParticles, check
    rt = eng.hreal
    out = dict(xtra1=np.empty(n, np.float64), ytra1=np.empty(n, np.float64), ztra1=np.empty(n, rt), itra1=np.empty(n, np.int32),
               npoint=np.empty(n, np.int32))
    p = FpxParticles()
    for k, a in out.items():
        setattr(p, k, a.ctypes.data)
    best = []
    for _ in range(3):
        eng.sync()
        t0 = time.perf_counter()
        check(eng.lib.fpx_download_particles(eng.h, 0, n, C.byref(p)), "fpx_download_particles")
        best.append((time.perf_counter() - t0) * 1e3)
    return out, min(best)


def run(n, real, numpoint, calls):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = scenario()
    sc["numpoint"] = numpoint
    sc["xmass"] = np.ones((1, numpoint))
    sc["npart_rel"] = np.full(numpoint, max(n // numpoint, 1), np.int32)
    eng = Engine(sc, compute_real_bytes=real, host_real_bytes=real, rng_mode=RNG_PHILOX, seed=0x5EED, max_particles=n, global_particles=n)
    eng.upload_diag_fields_from_scenario(sc)
    eng.seed_particles(n, seed=0x5EED, frac_pbl=0.5)
    arr, dl_ms = positions(eng, n)
    if numpoint > 1:                                  # the seeded cloud belongs to point 1: spread it over the points
        arr["npoint"] = (1 + np.arange(n) % numpoint).astype(np.int32)
        arr["npart"] = n
        eng.upload_particles_from_scenario(arr)
    eng.plumetraj_init(np.zeros(numpoint, np.int32), np.full(numpoint, 900, np.int32))
    ms, sweep_ms, sweeps = [], [], 0
    for i in range(calls + 1):                        # the first call pays for the code objects and the buffers
        nrec = eng.plumetraj(0)
        if i:
            ms.append(eng.plumetraj_time())
            sweep_ms.append(eng.info("plumetraj_sweep_us") / 1000.0)
            sweeps = eng.info("plumetraj_sweeps")
    rec = eng.get_plumetraj()
    eng.close()
    return dict(numpoint=numpoint, records=nrec, ms_per_call=float(np.median(ms)), ms_all=ms, sweep_loop_ms=float(np.median(sweep_ms)),
                sweep_share=float(np.median(sweep_ms) / np.median(ms)), max_sweeps=int(sweeps), sweeps_of_point_1=int(rec["iterations"][0]),
                download_ms=dl_ms, download_bytes=28 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_plumetraj: no GPU -- nothing is measured without one")
    n = int(a.particles)
    rows = [run(n, a.real, k, a.calls) for k in (1, 100)]
    out = {"metric": "plumetraj: device time of one fpx_plumetraj call, one release point", "unit": "ms", "higher_is_better": False,
           "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic", "value": rows[0]["ms_per_call"],
           "config": {"workload": f"{n:.0e} particles, 361x181x138, ncluster 5", "calls": a.calls}, "one_point": rows[0], "hundred_points": rows[1]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
