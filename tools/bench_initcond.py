#!/usr/bin/env python3
"""Measures the two kernels of the sensitivity to initial conditions (fpx_config.device_initcond; k_initcond and
k_initcond_finish) on one MI355X: a backward run of BASELINE config 4 (361x181x138 met grid, 360x180x10
output grid, CBL turbulence) with the option off and on, alternating in one process on the same seeded cloud.
  (a) k_initcond per step, by events of its own (fpx_initcond_time), next to the step with linit_cond = 0;
  (b) k_initcond_finish once over the whole cloud, next to k_conccalc (fpx_conccalc, ind_samp = 0) on the same cloud and
      output grid: the same scatter pattern.  Both are timed on the host around a synchronised call; the finish also by
      its events.
Prints ONE JSON line per particle count and, with --out, writes it to that file.
    python tools/bench_initcond.py [--particles 1e7 --real 8 --linit-cond 1 --steps 4 --warmup 2 --rounds 2 --out profiles/r10/initcond_1e7_f64.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scenario(nsteps, linit_cond):
    from flexpart_amd import synthetic as syn
    sc = syn.base_scenario(ctl=5.0, ifine=4, cblflag=1, nsteps=nsteps, ldirect=-1)
    sc["npart"] = 1
    sc["itramem"] = np.zeros(1, np.int32)
    sc["itime0"] = 0
    syn.add_outgrid(sc, nxg=360, nyg=180, nzg=10, outlon0=-180.0, outlat0=-90.0, dxout=1.0, dyout=1.0, ind_samp=0, old_fraction=0.0)
    del sc["npart"], sc["itramem"]
    if linit_cond:
        sc.update(linit_cond=linit_cond, device_initcond=1)
    return sc


def run(n, real, steps, warmup, linit_cond):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = scenario(steps + warmup, linit_cond)
    sc["npart_rel"] = np.array([n], np.int32)
    eng = Engine(sc, compute_real_bytes=real, host_real_bytes=real, rng_mode=RNG_PHILOX, seed=0x5EED, max_particles=n, sort_interval=4,
                 global_particles=n)
    eng.seed_particles(n, seed=0x5EED, frac_pbl=0.5)
    eng.sort()
    lsync = int(sc["lsynctime"])

    def do_step(i):
        itime = i * lsync
        w0 = -(abs(itime) // 10800) * 10800
        eng.set_windtime((w0, w0 - 10800), (1, 2))
        eng.step_async(itime)

    for i in range(warmup):
        do_step(i)
    eng.sync()
    eng.kernel_times(reset=True)
    if linit_cond:
        eng.initcond_time(reset=True)
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        do_step(i)
    eng.sync()
    wall = (time.perf_counter() - t0) / steps
    parts, launches = eng.kernel_times()
    res = dict(step_wall_ms=wall * 1e3, kernels_ms_per_step=[p / max(launches, 1) for p in parts])
    itime = (warmup + steps) * lsync
    conc = []
    for _ in range(3):                               # the first call pays for the code object
        eng.sync()
        t0 = time.perf_counter()
        eng.conccalc(itime, 1.0)
        eng.sync()
        conc.append((time.perf_counter() - t0) * 1e3)
    res["conccalc_wall_ms"] = min(conc)
    if linit_cond:
        ms, k = eng.initcond_time(reset=True)
        res.update(initcond_ms_per_step=ms / max(k, 1), initcond_steps=k)
        fin_wall, fin_dev = [], []
        for _ in range(3):
            eng.sync()
            t0 = time.perf_counter()
            eng.initcond_finish(itime)
            fin_wall.append((time.perf_counter() - t0) * 1e3)
            fin_dev.append(eng.initcond_time(reset=True)[0])
        grid = eng.get_initcond()
        res.update(finish_wall_ms=min(fin_wall), finish_device_ms=min(fin_dev), cells_set=int(np.count_nonzero(grid)),
                   grid_sum=float(grid.astype(np.float64).sum()))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--linit-cond", type=int, default=1, choices=(1, 2))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--off-only", action="store_true", help="measure only the step without the option (also runs on a commit without it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_initcond: no GPU -- nothing is measured without one")
    n = int(a.particles)
    off, on = [], []
    for _ in range(a.rounds):                       # alternate the two versions in one call
        off.append(run(n, a.real, a.steps, a.warmup, 0))
        if not a.off_only:
            on.append(run(n, a.real, a.steps, a.warmup, a.linit_cond))
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    cfg = {"workload": f"{n:.0e} particles, backward run of config 4 (361x181x138, CBL), output grid 360x180x10, one species",
           "linit_cond": a.linit_cond, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
    out = {"metric": "initcond: device time of k_initcond_finish over the whole cloud", "unit": "ms", "higher_is_better": False,
           "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic", "config": cfg,
           "step_wall_ms_device_initcond_off": med(off, "step_wall_ms"), "conccalc_wall_ms_off": med(off, "conccalc_wall_ms"),
           "step_wall_ms_all": {"off": [r["step_wall_ms"] for r in off], "on": [r["step_wall_ms"] for r in on]},
           "kernels_ms_per_step_off": off[-1]["kernels_ms_per_step"]}
    if a.off_only:
        out.update(metric="initcond: wall time of the step with device_initcond off", value=out["step_wall_ms_device_initcond_off"])
    else:
        out.update(value=med(on, "finish_device_ms"), step_wall_ms_device_initcond_on=med(on, "step_wall_ms"),
                   initcond_ms_per_step=med(on, "initcond_ms_per_step"), finish_wall_ms=med(on, "finish_wall_ms"),
                   conccalc_wall_ms_on=med(on, "conccalc_wall_ms"), finish_over_conccalc=med(on, "finish_wall_ms") / med(on, "conccalc_wall_ms"),
                   initcond_over_step=med(on, "initcond_ms_per_step") / med(off, "step_wall_ms"),
                   cells_set=on[-1]["cells_set"], grid_sum=on[-1]["grid_sum"], kernels_ms_per_step_on=on[-1]["kernels_ms_per_step"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
