#!/usr/bin/env python3
"""Measures the gross-flux kernels (fpx_config.device_flux; k_flux_save + k_calcfluxes) on one MI355X:
the particle step of BASELINE config 4 (361x181x138 met grid, 360x180x10 output grid, CBL turbulence) with device_flux off
and on, alternating in one process on the same seeded cloud, and the two kernels by events of their own
(fpx_calcfluxes_time).  Prints ONE JSON line per particle count and, with --out, writes it to that file.
    python tools/bench_calcfluxes.py [--particles 1e7 --real 8 --steps 4 --warmup 2 --rounds 2 --out profiles/r5/calcfluxes_1e7.json]
The bytes model: k_flux_save reads itra1, xt, yt, zt, xmass1 and writes xold, yold, zold, the masses and the due mark;
k_calcfluxes reads those back with xt, yt, zt, npoint, itramem.  The atomics on the faces crossed are not in it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def scenario(nsteps, on):
    from flexpart_amd import synthetic as syn
    sc = syn.base_scenario(ctl=5.0, ifine=4, cblflag=1, nsteps=nsteps)
    sc["npart"] = 1
    sc["itramem"] = np.zeros(1, np.int32)
    sc["itime0"] = 0
    syn.add_outgrid(sc, nxg=360, nyg=180, nzg=10, outlon0=-180.0, outlat0=-90.0, dxout=1.0, dyout=1.0, ind_samp=-1, old_fraction=0.0)
    del sc["npart"], sc["itramem"]
    if on:
        sc.update(iflux=1, device_flux=1)
    return sc


def bytes_per_particle(rb, hb, nspec=1):
    save = 4 + 16 + rb + nspec * rb + 3 * hb + nspec * hb + 1
    calc = 1 + 3 * hb + nspec * hb + 16 + rb + 8
    return save + calc


def run(n, real, steps, warmup, on):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = scenario(steps + warmup, on)
    sc["npart_rel"] = np.array([n], np.int32)
    eng = Engine(sc, compute_real_bytes=real, host_real_bytes=real, rng_mode=RNG_PHILOX, seed=0x5EED, max_particles=n, sort_interval=4,
                 global_particles=n)
    eng.seed_particles(n, seed=0x5EED, frac_pbl=0.5)
    eng.sort()
    lsync = int(sc["lsynctime"])

    def do_step(i):
        itime = i * lsync
        w0 = (itime // 10800) * 10800
        eng.set_windtime((w0, w0 + 10800), (1, 2))
        eng.step_async(itime)

    for i in range(warmup):
        do_step(i)
    eng.sync()
    eng.kernel_times(reset=True)
    if on:
        eng.calcfluxes_time(reset=True)
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        do_step(i)
    eng.sync()
    wall = (time.perf_counter() - t0) / steps
    parts, launches = eng.kernel_times()
    res = dict(step_wall_ms=wall * 1e3, kernels_ms_per_step=[p / max(launches, 1) for p in parts])
    if on:
        ms, k = eng.calcfluxes_time()
        flux = eng.get_flux()
        res.update(flux_kernels_ms_per_step=ms / max(k, 1), flux_steps=k, flux_cells_set=int(np.count_nonzero(flux)),
                   flux_sum=float(flux.astype(np.float64).sum()), flux_bytes=int(flux.nbytes))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_calcfluxes: no GPU -- nothing is measured without one")
    n = int(a.particles)
    off, on = [], []
    for _ in range(a.rounds):                       # alternate the two versions in one call
        off.append(run(n, a.real, a.steps, a.warmup, False))
        on.append(run(n, a.real, a.steps, a.warmup, True))
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    t_off, t_on, t_flux = med(off, "step_wall_ms"), med(on, "step_wall_ms"), med(on, "flux_kernels_ms_per_step")
    bpp = bytes_per_particle(a.real, a.real)
    gbs = bpp * n / (t_flux * 1e-3) / 1e9
    out = {"metric": "calcfluxes: device time of k_flux_save + k_calcfluxes per step", "value": t_flux, "unit": "ms", "higher_is_better": False,
           "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic",
           "config": {"workload": f"{n:.0e} particles, config 4 (361x181x138, CBL), output grid 360x180x10, one species", "steps": a.steps,
                      "warmup": a.warmup, "rounds": a.rounds},
           "step_wall_ms_device_flux_off": t_off, "step_wall_ms_device_flux_on": t_on, "step_wall_ms_all": {"off": [r["step_wall_ms"] for r in off],
                                                                                                          "on": [r["step_wall_ms"] for r in on]},
           "added_fraction_of_step": (t_on - t_off) / t_off, "flux_kernels_over_step": t_flux / t_off,
           "flux_cells_set": on[-1]["flux_cells_set"], "flux_sum": on[-1]["flux_sum"], "flux_bytes": on[-1]["flux_bytes"],
           "kernels_ms_per_step_off": off[-1]["kernels_ms_per_step"], "kernels_ms_per_step_on": on[-1]["kernels_ms_per_step"],
           "roofline": {"bound": "hbm", "alg_bytes_per_particle": bpp, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                        "kernel": "k_flux_save + k_calcfluxes"}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
