#!/usr/bin/env python3
"""Measures the OH reaction (fpx_ohreaction: k_oh_blend + k_ohreaction) on one MI355X: a seeded, sorted cloud
on the 361x181x138 met grid, an OH grid of 72 x 46 x 7 (5 x 4 degrees, seven levels: the shape of the climatology the
reference's OH_FIELDS/OH_variables.bin holds; --ohgrid takes another), one and three reacting species; --dark sets OH to 0
everywhere, which leaves the state loads, the searches and the OH gather.  The device time is
that of the two kernels by events of their own (fpx_ohreaction_time), the median of --calls calls after --warmup.  On the same
run it times what the call makes unnecessary: xtra1, ytra1, ztra1, itra1 and xmass1 down to the host and up again (the
upload call takes the positions along with the masses).
Prints ONE JSON line and, with --out, writes it to that file.
    python tools/bench_ohreaction.py [--particles 1e7 --real 8 --calls 20 --warmup 3 --out profiles/r16/ohreaction_1e7_f64.json]
The bytes model (compulsory traffic): per particle xtra1, ytra1 (8 + 8), ztra1 (R), itra1 (4), one tt and one OH value
gathered (H each; counted per particle, an upper bound: neighbours share cache lines), and per reacting species xmass1 read
and written (2 R)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_GBS = 6300.0


def oh_arrays(nxo, nyo, nzo, nspec):
    """A lit, positive climatology of the given shape (every particle reacts: the worst case for the kernel)."""
    m, k, j, i = np.meshgrid(np.arange(12), np.arange(nzo), np.arange(nyo), np.arange(nxo), indexing="ij")
    alt = 500.0 * (1.0 + np.arange(nzo)) ** 1.6
    return dict(lonOH=-180.0 + (360.0 / nxo) * (np.arange(nxo) + 0.5), latOH=-90.0 + (180.0 / nyo) * (np.arange(nyo) + 0.5), altOH=alt,
                OH_field=1.0e6 * (1.0 + ((i * 5 + j * 3 + k * 7 + m * 2) % 11) / 16.0), jrate_average=np.full((12, 180, 360), 2.0e-5),
                lonjr=-179.5 + np.arange(360.0), latjr=-89.5 + np.arange(180.0), bdate=2458864.5,
                ohcconst=np.array([1.0e-13, 1.0e-14, 2.0e-14, 0.0, 0.0])[:nspec], ohdconst=np.array([1200.0, -300.0, 500.0, 0.0, 0.0])[:nspec],
                ohnconst=np.array([2.0, 1.5, 0.5, 0.0, 0.0])[:nspec])


def run(n, real, nspec, ohgrid, calls, warmup, dark=False):
    from flexpart_amd import synthetic as syn
    from flexpart_amd._lib import FpxParticles, check
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = syn.base_scenario(ctl=5.0, ifine=4, cblflag=1, nsteps=1, nspec=nspec)
    eng = Engine(sc, compute_real_bytes=real, host_real_bytes=real, rng_mode=RNG_PHILOX, seed=0x5EED, max_particles=n, global_particles=n)
    eng.seed_particles(n, seed=0x5EED, frac_pbl=0.5)
    eng.sort()
    eng.upload_tt(sc["tt"])
    c = oh_arrays(*ohgrid, nspec)
    eng.oh_init(c)
    eng.gethourlyOH(0)
    oh, _ = eng.get_oh_hourly()
    lit = 0.0 if dark else 1.0                             # dark: OH exactly 0, no particle reacts
    eng.set_oh_hourly(np.stack([np.maximum(oh[0], 1.0e5) * lit, np.maximum(oh[1], 1.0e5) * lit]), (0.0, 3600.0))
    eng.set_windtime((0, 10800), (1, 2))
    ms = []
    for i in range(warmup + calls):
        eng.ohreaction(900, 900)
        t = eng.ohreaction_time()
        if i >= warmup:
            ms.append(t)
    skipped = eng.info("oh_skipped")
    # the round trip the call replaces
    rt = np.float32 if real == 4 else np.float64
    x, y, z, it, m = np.empty(n), np.empty(n), np.empty(n, rt), np.empty(n, np.int32), np.empty((nspec, n), rt)
    p = FpxParticles()                     # (fpx_upload_particles takes the positions and itra1 along with the masses)
    p.xtra1, p.ytra1, p.ztra1, p.itra1, p.xmass1, p.xmass1_ld = x.ctypes.data, y.ctypes.data, z.ctypes.data, it.ctypes.data, m.ctypes.data, n
    copy = []
    for _ in range(3):
        eng.sync()
        t0 = time.perf_counter()
        check(eng.lib.fpx_download_particles(eng.h, 0, n, C.byref(p)), "fpx_download_particles")
        check(eng.lib.fpx_upload_particles(eng.h, 0, n, C.byref(p)), "fpx_upload_particles")
        eng.sync()
        copy.append((time.perf_counter() - t0) * 1e3)
    reacted = float((m[0] > 0).mean())
    eng.close()
    return dict(ms=ms, copy_ms=copy, skipped=skipped, alive_fraction=reacted)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ohgrid", default="72,46,7")
    ap.add_argument("--dark", action="store_true", help="OH = 0 everywhere: the kernel without the tt gather, pow, exp and the mass stores")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ohreaction: no GPU -- nothing is measured without one")
    n = int(a.particles)
    ohgrid = tuple(int(v) for v in a.ohgrid.split(","))
    rows = {}
    for nspec in (1, 3):
        r = run(n, a.real, nspec, ohgrid, a.calls, a.warmup, a.dark)
        t = float(np.median(r["ms"]))
        bpp = 16 + a.real + 4 + 2 * a.real + nspec * 2 * a.real
        gbs = n * bpp / (t * 1e-3) / 1e9
        rows[f"species_{nspec}"] = dict(device_ms=t, device_ms_min=float(min(r["ms"])), device_ms_max=float(max(r["ms"])), alg_bytes_per_particle=bpp,
                                        achieved_gbs=gbs, frac_of_achievable_hbm=gbs / HBM_ACHIEVABLE_GBS, host_round_trip_ms=float(np.median(r["copy_ms"])),
                                        oh_skipped=r["skipped"])
    out = {"metric": "ohreaction: device time of k_oh_blend + k_ohreaction, three reacting species", "value": rows["species_3"]["device_ms"], "unit": "ms",
           "higher_is_better": False, "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic",
           "config": {"workload": f"{n:.0e} particles sorted on 361x181x138, OH grid {ohgrid[0]}x{ohgrid[1]}x{ohgrid[2]}, " + ("no particle reacts (--dark)" if a.dark else "every particle reacts"), "calls": a.calls, "warmup": a.warmup},
           "rows": rows, "roofline": {"bound": "hbm", "achievable": HBM_ACHIEVABLE_GBS, "unit": "GB/s", "kernel": "k_ohreaction"}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
