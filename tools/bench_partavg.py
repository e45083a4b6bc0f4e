#!/usr/bin/env python3
"""Measures the interval-average kernel (fpx_config.device_partavg; k_partavg) on one MI355X: the
particle step of BASELINE config 4 (361x181x138 met grid, 360x180x10 output grid, CBL turbulence) with the option off and
on, alternating in one process on the same seeded cloud, and the kernel by events of its own (fpx_partavg_time).  Prints
ONE JSON line per particle count and, with --out, writes it to that file.
    python tools/bench_partavg.py [--particles 1e7 --real 8 --steps 4 --warmup 2 --rounds 2 --out profiles/r6/partavg_1e7_f64.json]
The bytes model (compulsory traffic): per due particle the fifteen values read and written, the position and the key of
k_prep; the gathers counted once as the bytes of the packs they read (uu/vv/ww, rho/drhodz, pv/qv/tt of both slots, the
surface pack, oro and the two tropopause fields)."""
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
    if on:
        syn.add_partoutput_fields(sc, itime=0, dead_every=0)
        del sc["itra1"], sc["npoint"]
        sc.update(ipout=3, device_partavg=1)
    del sc["npart"], sc["itramem"]
    return sc


def model_bytes(n, rb, hb, grid):
    nx, ny, nz = grid
    per_particle = 2 * (4 + 14 * hb) + 16 + rb + 1
    packs = nx * ny * nz * (6 * rb + 4 * rb + 6 * hb) + nx * ny * (8 * rb + 3 * hb)
    return per_particle, packs, n * per_particle + packs


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
        eng.partavg_time(reset=True)
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        do_step(i)
    eng.sync()
    wall = (time.perf_counter() - t0) / steps
    parts, launches = eng.kernel_times()
    res = dict(step_wall_ms=wall * 1e3, kernels_ms_per_step=[p / max(launches, 1) for p in parts])
    if on:
        ms, k = eng.partavg_time()
        head = eng.get_partavg(0, min(n, 100000))
        res.update(partavg_ms_per_step=ms / max(k, 1), partavg_steps=k, npart_av_max=int(head["npart_av"].max()),
                   mean_tt=float(np.mean(head["tt"].astype(np.float64) / np.maximum(head["npart_av"], 1))))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--off-only", action="store_true", help="measure only the step without the option (also runs on a commit without it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_partavg: no GPU -- nothing is measured without one")
    n = int(a.particles)
    off, on = [], []
    for _ in range(a.rounds):                       # alternate the two versions in one call
        off.append(run(n, a.real, a.steps, a.warmup, False))
        if not a.off_only:
            on.append(run(n, a.real, a.steps, a.warmup, True))
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    t_off = med(off, "step_wall_ms")
    cfg = {"workload": f"{n:.0e} particles, config 4 (361x181x138, CBL), output grid 360x180x10, one species", "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds}
    if a.off_only:
        out = {"metric": "partavg: wall time of the step with device_partavg off", "value": t_off, "unit": "ms", "higher_is_better": False,
               "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic", "config": cfg,
               "step_wall_ms_all": {"off": [r["step_wall_ms"] for r in off]}, "kernels_ms_per_step_off": off[-1]["kernels_ms_per_step"]}
    else:
        t_on, t_pa = med(on, "step_wall_ms"), med(on, "partavg_ms_per_step")
        bpp, packs, total = model_bytes(n, a.real, a.real, (361, 181, 138))
        gbs = total / (t_pa * 1e-3) / 1e9
        out = {"metric": "partavg: device time of k_partavg per step", "value": t_pa, "unit": "ms", "higher_is_better": False,
               "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic", "config": cfg,
               "step_wall_ms_device_partavg_off": t_off, "step_wall_ms_device_partavg_on": t_on,
               "step_wall_ms_all": {"off": [r["step_wall_ms"] for r in off], "on": [r["step_wall_ms"] for r in on]},
               "added_fraction_of_step": (t_on - t_off) / t_off, "partavg_over_step": t_pa / t_off,
               "npart_av_max": on[-1]["npart_av_max"], "mean_tt": on[-1]["mean_tt"],
               "kernels_ms_per_step_off": off[-1]["kernels_ms_per_step"], "kernels_ms_per_step_on": on[-1]["kernels_ms_per_step"],
               "roofline": {"bound": "hbm", "alg_bytes_per_particle": bpp, "pack_bytes": packs, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": gbs / HBM_PEAK_GBS, "kernel": "k_partavg"}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
