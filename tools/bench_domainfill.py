#!/usr/bin/env python3
"""Measures fpx_boundcond_domainfill (boundary conditions of a domain-filling run) on one MI355X:
361x181x138 met grid, a limited-area filling box nx_we = (1, 358), ny_sn = (5, 175) that keeps nearly every particle of the
seeded cloud alive, columns of 20 release heights on all four boundaries, counter RNG, warmed up.  Per call: the device
time by the call's own events (fpx_domainfill_time) and its split over the stages (fpx_get_info), the candidates, and the
rate of the full-space pass against its 20 bytes per storage space.  In the same run it times what a host without the
feature pays every step: fpx_download_particles of itra1, xtra1, ytra1 and the way back (fpx_upload_particles, which also
takes ztra1).
Prints ONE JSON line and, with --out, writes it to that file.
    python tools/bench_domainfill.py [--particles 1e7 --real 8 --calls 5 --out profiles/r12/domainfill_1e7_f64.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NCOL = 20


def scenario(xmpp):
    from flexpart_amd import synthetic as syn
    sc = syn.base_scenario(ctl=5.0, ifine=4, cblflag=0, nsteps=1)
    sc["npart"] = 1
    syn.add_partoutput_fields(sc, itime=0, dead_every=0)
    sc["pv"] = sc["pv"] * 2.0e6
    for k in ("npart", "itra1", "npoint"):
        del sc[k]
    nx, ny, _ = (int(v) for v in sc["grid"])
    sc["mdomainfill"] = 1
    sc["nx_we"], sc["ny_sn"] = np.array([1, nx - 3], np.int32), np.array([5, ny - 6], np.int32)
    sc["xmassperparticle"], sc["nclassunc"], sc["itsplit"] = xmpp, 1, 999999999
    z = 250.0 + 750.0 * np.arange(NCOL, dtype=np.float64)[:, None, None]
    for side, nrow in (("we", ny), ("sn", nx)):
        sc["numcolumn_" + side] = np.full((nrow, 2), NCOL, np.int32)
        sc["zcolumn_" + side] = z + np.zeros((NCOL, nrow, 2))
        sc["acc_mass_" + side] = np.zeros((NCOL, nrow, 2))
    return sc


def copies(eng, n):
    """(download ms, upload ms): best wall time of three each."""
    from flexpart_amd._lib import FpxParticles, check
    rt = eng.hreal
    a = dict(xtra1=np.empty(n, np.float64), ytra1=np.empty(n, np.float64), itra1=np.empty(n, np.int32))
    p = FpxParticles()
    for k, v in a.items():
        setattr(p, k, v.ctypes.data)
    down, up = [], []
    for _ in range(3):
        eng.sync()
        t0 = time.perf_counter()
        check(eng.lib.fpx_download_particles(eng.h, 0, n, C.byref(p)), "fpx_download_particles")
        down.append((time.perf_counter() - t0) * 1e3)
    a["ztra1"] = np.full(n, 100.0, rt)
    p.ztra1 = a["ztra1"].ctypes.data
    for _ in range(3):
        eng.sync()
        t0 = time.perf_counter()
        check(eng.lib.fpx_upload_particles(eng.h, 0, n, C.byref(p)), "fpx_upload_particles")
        up.append((time.perf_counter() - t0) * 1e3)
    return min(down), min(up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=float, default=1e7)
    ap.add_argument("--real", type=int, default=8, choices=(4, 8))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--xmpp", type=float, default=3.0e12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_domainfill: no GPU -- nothing is measured without one")
    from flexpart_amd.engine import Engine, RNG_PHILOX
    n = int(a.particles)
    sc = scenario(a.xmpp)
    eng = Engine(sc, compute_real_bytes=a.real, host_real_bytes=a.real, rng_mode=RNG_PHILOX, seed=0x5EED, max_particles=n + n // 10, global_particles=n)
    eng.upload_diag_fields_from_scenario(sc)
    eng.seed_particles(n, seed=0x5EED, frac_pbl=0.5)
    eng.domainfill_init(sc)
    rows = []
    for i in range(a.calls + 2):                      # the first call terminates what the seed put outside and pays for the buffers
        st = eng.boundcond_domainfill(0)
        if i >= 2:
            rows.append(dict(ms=eng.domainfill_time(), candidates=int(eng.info("domainfill_candidates")), released=int(st["n_released"]),
                             terminated=int(st["n_terminated"]), active=int(st["numactiveparticles"]), numpart=eng.n,
                             **{k: eng.info(f"domainfill_{k}_us") / 1000.0 for k in ("flux", "stage1", "cand", "place")}))
    numpart = eng.n
    down, up = copies(eng, numpart)
    eng.close()
    med = lambda k: float(np.median([r[k] for r in rows]))
    out = {"metric": "boundcond_domainfill: device time of one fpx_boundcond_domainfill call", "unit": "ms", "higher_is_better": False,
           "dtype": "f64" if a.real == 8 else "f32", "data": "synthetic", "value": med("ms"),
           "config": {"workload": f"{n:.0e} particles, 361x181x138, box (1,358)x(5,175), {NCOL} heights per column", "calls": a.calls,
                      "locations": 2 * NCOL * ((sc['ny_sn'][1] - sc['ny_sn'][0] + 1) + (sc['nx_we'][1] - sc['nx_we'][0] + 1)).item()},
           "stages_ms": {k: med(k) for k in ("flux", "stage1", "cand", "place")}, "candidates_per_call": med("candidates"),
           "storage_spaces": numpart, "stage1_GBps_of_20B_per_space": 20.0 * numpart / (med("stage1") * 1e-3) / 1e9 if med("stage1") > 0 else None,
           "host_copy_ms": {"download_itra1_xtra1_ytra1": down, "upload_back_with_ztra1": up, "bytes_down": 20 * numpart}, "calls": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
