"""Host-side mirror of the reference's particle loop, on top of the C ABI.

`Engine` plays the role of the Fortran host around the replaced block
(reference src/timemanager.f90:531-712): it owns com_mod-shaped host arrays,
hands them to the GPU engine through include/flexpart_amd.h, and exposes the
same vocabulary (xtra1, ytra1, ztra1, uap, ucp, uzp, us, vs, ws, idt, itra1,
itramem, cbt, xmass1; memtime/memind; lsynctime ...).  All arithmetic happens
in the HIP library; nothing here computes trajectories.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (FpxConfig, FpxFields, FpxNests, FpxOutgrid, FpxOutgridNest, FpxParticles, FpxStepStats, FpxWetConfig, FpxWetFields, RNG_PHILOX,
                   RNG_TABLE_COUNTER, RNG_TABLE_SEQ, check)

# polar stereographic set-up is host work in the reference (gridcheck_ecmwf.f90:341-366 via
# cmapf_mod stlmbr/stcm2p); the engine only consumes the resulting 9-number map records.
SWITCHNORTH, SWITCHSOUTH = 75.0, -75.0


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def release_tables(sc):
    """(xmass [nspec][numpoint], npart [numpoint]) of a scenario: keys numpoint, xmass, npart_rel; the default is
    the single release point of unit mass holding every particle."""
    nspec = int(sc["nspec"])
    numpoint = int(sc.get("numpoint", 1))
    xm = np.asarray(sc.get("xmass", np.ones(nspec * numpoint)), dtype=np.float64).reshape(nspec, numpoint)
    npt = np.asarray(sc.get("npart_rel", np.full(numpoint, max(int(sc.get("npart", 0)), 1))), dtype=np.int32).ravel()
    return xm, npt


class Engine:
    def __init__(self, sc, *, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_TABLE_SEQ,
                 seed=0x5EED, max_particles=None, device=0, pad=(0, 0, 0), sort_interval=0,
                 polemaps=None, particle_base=0, blend_mode=0, global_particles=0, pbl_slice_passes=0, options=None,
                 nest_pad=(0, 0)):
        """sc: scenario dict (flexpart_amd.synthetic).  pad: extra allocated (nxmax-nx,
        nymax-ny, nzmax-nz) to exercise the reference's padded-array convention; nest_pad: the
        same for the nested wind fields (nxmaxn-nxn, nymaxn-nyn)."""
        self.lib = _lib.load()
        self.sc = sc
        self.hreal = np.float32 if host_real_bytes == 4 else np.float64
        nx, ny, nz = (int(v) for v in sc["grid"])
        self.nx, self.ny, self.nz = nx, ny, nz
        self.nxmax, self.nymax, self.nzmax = nx + pad[0], ny + pad[1], nz + pad[2]
        self.nest_pad = (int(nest_pad[0]), int(nest_pad[1]))
        self._nest_extent = (0, 0)                      # nxn, nyn of nest 1 once init_nest has run
        self._nest_extents = []                         # nxn, nyn of every nest (init_nest, init_nests)
        self._nest_max = None                           # nxmaxn, nymaxn
        dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
        xg, ng, sg = (int(v) for v in sc["globalflags"])
        nspec = int(sc["nspec"])
        self.nspec = nspec
        n = int(sc.get("npart", 0))
        cfg = FpxConfig()
        cfg.struct_bytes = C.sizeof(FpxConfig)
        cfg.device = device
        cfg.compute_real_bytes = compute_real_bytes
        cfg.host_real_bytes = host_real_bytes
        cfg.max_particles = int(max_particles or max(n, 1))
        cfg.nx, cfg.ny, cfg.nz, cfg.nmixz = nx, ny, nz, int(sc.get("nmixz", nz))   # without height/nmixz: set by verttransform(init)
        cfg.nxmax, cfg.nymax, cfg.nzmax = self.nxmax, self.nymax, self.nzmax
        cfg.dx, cfg.dy, cfg.xlon0, cfg.ylat0 = dx, dy, xlon0, ylat0
        cfg.xglobal, cfg.nglobal, cfg.sglobal = xg, ng, sg
        rt = self.hreal
        # (switchnorth-ylat0)/dy in the host's default real kind, gridcheck_ecmwf.f90:348,362
        cfg.switchnorthg = float((rt(SWITCHNORTH) - rt(ylat0)) / rt(dy)) if ng else 999999.0
        cfg.switchsouthg = float((rt(SWITCHSOUTH) - rt(ylat0)) / rt(dy)) if sg else 999999.0
        if ng or sg:
            if polemaps is None:   # the host has no com_mod records: build them as gridcheck does
                north = (C.c_double * 9)()
                south = (C.c_double * 9)()
                check(self.lib.fpx_polar_maps(host_real_bytes, dy, north, south), "fpx_polar_maps")
                polemaps = (list(north), list(south))
            for i in range(9):
                cfg.northpolemap[i] = float(polemaps[0][i])
                cfg.southpolemap[i] = float(polemaps[1][i])
        for k in ("ldirect", "lsynctime", "method", "mintime", "ifine", "turbswitch", "cblflag",
                  "mdomainfill", "lsettling"):
            setattr(cfg, k, int(sc[k]))
        cfg.ctl = float(sc["ctl"])
        cfg.d_trop, cfg.d_strat, cfg.turbmesoscale = (float(v) for v in sc["turbpar"])
        cfg.nspec = nspec
        cfg.maxspec = nspec
        cfg.drydep = int(sc["drydep"])
        for i in range(nspec):
            cfg.drydepspec[i] = int(np.asarray(sc["drydepspec"]).ravel()[i])
            cfg.density[i] = float(sc["density"][i]); cfg.dquer[i] = float(sc["dquer"][i])
            cfg.vsetaver[i] = float(sc["vsetaver"][i]); cfg.cunningham[i] = float(sc["cunningham"][i])
            cfg.decay[i] = float(sc["decay"][i])
        cfg.mquasilag = int(sc.get("mquasilag", 0))
        cfg.lage_last = int(np.asarray(sc["lage"]).ravel()[-1])
        cfg.rng_mode = rng_mode
        cfg.seed = seed
        cfg.sort_interval = sort_interval
        # eps = nxmax/3.e5 uses the par_mod nxmax of the host build (advance.f90:107); scenarios carry
        # it so that runs compare with the reference binary they were pinned against (361 or 721)
        cfg.par_nxmax = int(sc.get("par_nxmax", 361))
        cfg.particle_base = int(particle_base or sc.get("particle_base", 0))
        cfg.drybkdep, cfg.wetbkdep = int(sc.get("drybkdep", 0)), int(sc.get("wetbkdep", 0))   # backward runs with receptor scavenging
        self.bkdep = bool(cfg.drybkdep or cfg.wetbkdep)
        cfg.turboff, cfg.interpolhmix = int(sc.get("turboff", 0)), int(sc.get("interpolhmix", 0))   # com_mod.f90:777-778
        cfg.ipout, cfg.iflux, cfg.linit_cond = int(sc.get("ipout", 0)), int(sc.get("iflux", 0)), int(sc.get("linit_cond", 0))   # refused when set
        cfg.device_flux = int(sc.get("device_flux", 0))   # iflux = 1 is accepted with it: the fluxes are computed here (get_flux, fluxoutput)
        cfg.device_initcond = int(sc.get("device_initcond", 0))   # linit_cond = 1, 2 is accepted with it: init_cond is summed here (initcond_finish, get_initcond, initial_cond_output)
        cfg.device_partavg = int(sc.get("device_partavg", 0))   # ipout = 3 is accepted with it: the interval averages are kept here (get_partavg, partoutput_average)
        cfg.blend_mode = int(blend_mode)                # 0: from global_particles, 1 on, 2 off
        cfg.global_particles = int(global_particles)    # the run's particle count over all ranks
        cfg.pbl_slice_passes = int(pbl_slice_passes)    # 0: the engine's schedule, -1: one launch, k: k passes per launch
        self.cfg = cfg
        self.h = C.c_void_p()
        check(self.lib.fpx_create(C.byref(self.h), C.byref(cfg)), "fpx_create")
        for name, value in (options or {}).items():
            self.set_option(name, value)
        if "height" in sc:
            hgt = np.ascontiguousarray(np.asarray(sc["height"]).astype(rt))
            check(self.lib.fpx_set_height(self.h, _vp(hgt), nz), "fpx_set_height")
        self.itime = int(sc.get("itime0", 0))
        self.lsynctime = int(sc["lsynctime"])
        self.n = 0
        self.set_release_points(*release_tables(sc))
        if "zpoint1" in sc and "zpoint2" in sc:      # point_mod zpoint1/zpoint2: WETBKDEP multiplies with the release's height range
            z1 = np.ascontiguousarray(np.asarray(sc["zpoint1"]).astype(rt))
            z2 = np.ascontiguousarray(np.asarray(sc["zpoint2"]).astype(rt))
            check(self.lib.fpx_set_release_heights(self.h, z1.size, _vp(z1), _vp(z2)), "fpx_set_release_heights")
        if rng_mode != RNG_PHILOX:
            check(self.lib.fpx_rng_fill_table(self.h), "fpx_rng_fill_table")
        if "uu" in sc:
            self.upload_fields_from_scenario(sc)
        if "nest" in sc:
            self.upload_nests_from_scenario(sc)
        if n:
            self.upload_particles_from_scenario(sc)
        if cfg.device_partavg and "pv" in sc and "oro" in sc:
            self.upload_diag_fields_from_scenario(sc)
        self.gshape = None
        if "outgrid" in sc:
            self.outgrid_from_scenario(sc)
        self.has_wet = bool(sc.get("wetdep", 0))
        self.has_conv = False                        # set by conv_init: run() then calls convmix where timemanager does
        if self.has_wet:
            self.wet_from_scenario(sc)

    # ---- met fields ---------------------------------------------------------
    def _host3(self, a, m):
        """slot m of a compact (2,nz,ny,nx) array -> com_mod-shaped padded host array."""
        out = np.zeros((self.nzmax, self.nymax, self.nxmax), self.hreal)
        out[: self.nz, : self.ny, : self.nx] = a[m]
        return out

    def _host2(self, a, m):
        out = np.zeros((self.nymax, self.nxmax), self.hreal)
        out[: self.ny, : self.nx] = a[m]
        return out

    def _nest_host(self, a, dtype=None, nlev=None):
        """compact [...][nyn][nxn] nest array -> the host's [...][nymaxn][nxmaxn] (nest_pad), the leading axis grown to nlev."""
        a = np.asarray(a)
        lead = a.shape[:-2] if nlev is None else (nlev,) + a.shape[1:-2]
        nxmaxn, nymaxn = self._nest_max or (a.shape[-1] + self.nest_pad[0], a.shape[-2] + self.nest_pad[1])   # one nxmaxn, nymaxn for all nests
        out = np.zeros(lead + (nymaxn, nxmaxn), dtype or self.hreal)
        out[tuple(slice(0, n) for n in a.shape)] = a
        return out

    def upload_fields_from_scenario(self, sc):
        for m in (0, 1):
            keep = {}
            f = FpxFields()
            for k in ("uu", "vv", "ww", "uupol", "vvpol", "rho", "drhodz", "tt"):
                if k in sc:
                    keep[k] = self._host3(sc[k], m)
                    setattr(f, k, keep[k].ctypes.data)
            for k in ("hmix", "ustar", "wstar", "oli", "tropopause"):
                keep[k] = self._host2(sc[k], m)
                setattr(f, k, keep[k].ctypes.data)
            if "vdep" in sc:
                v = np.zeros((self.nspec, self.nymax, self.nxmax), self.hreal)
                v[:, : self.ny, : self.nx] = sc["vdep"][m]
                keep["vdep"] = v
                f.vdep = v.ctypes.data
            check(self.lib.fpx_upload_fields(self.h, m + 1, C.byref(f)), "fpx_upload_fields")
        self.set_windtime(sc["memtime"], sc["memind"])

    def verttransform(self, slot, m, sfc, *, init=False, want=("uu", "vv", "ww", "tt", "qv", "pv", "rho", "drhodz", "uupol", "vvpol"),
                      host_arrays=None, nest=None, device_pv=False):
        """fpx_verttransform_ecmwf: m = synthetic.model_levels() dict (compact [nz][ny][nx] arrays),
        sfc = dict of compact 2-D fields (hmix, ustar, wstar, oli, tropopause[, vdep]) for this slot.
        device_pv: pvh = NULL, the potential vorticity is computed on the device (calcpv / calcpv_nests); m needs no pvh.
        Returns the z-level arrays asked for (compact), height and nmixz."""
        from ._lib import FpxModelLevels, FpxFieldsOut
        rt = self.hreal
        if nest is not None:      # m is the nest's input (synthetic.nest_model_levels): fpx_verttransform_nest of nest `nest` (1-based)
            return self._verttransform_nest(slot, m, sfc, want, device_pv, nest=int(nest))
        keep = {} if host_arrays is None else host_arrays     # host_arrays: a dict the caller keeps alive -> arrays stay put and are pinned
        ml = FpxModelLevels()
        ml.pin_host = 0 if host_arrays is None else 1
        for k in ("uuh", "vvh", "pvh", "wwh", "tth", "qvh"):
            if k == "pvh" and device_pv:
                continue
            if k not in keep:
                keep[k] = np.zeros((self.nzmax, self.nymax, self.nxmax), rt)
            keep[k][: self.nz, : self.ny, : self.nx] = m[k]
            setattr(ml, k, keep[k].ctypes.data)
        for k in ("ps", "tt2", "td2"):
            if k not in keep:
                keep[k] = np.zeros((self.nymax, self.nxmax), rt)
            keep[k][: self.ny, : self.nx] = m[k]
            setattr(ml, k, keep[k].ctypes.data)
        for k in ("akz", "bkz", "aknew", "bknew"):
            keep[k] = np.ascontiguousarray(np.asarray(m[k]).astype(rt))
            setattr(ml, k, keep[k].ctypes.data)
        ml.nuvz = ml.nwz = self.nz
        ml.init = int(init)
        f = FpxFields()
        for k in ("hmix", "ustar", "wstar", "oli", "tropopause"):
            if sfc is None:
                break
            a = np.zeros((self.nymax, self.nxmax), rt)
            a[: self.ny, : self.nx] = sfc[k]
            keep["s" + k] = a
            setattr(f, k, a.ctypes.data)
        if sfc is not None and "vdep" in sfc:
            v = np.zeros((self.nspec, self.nymax, self.nxmax), rt)
            v[:, : self.ny, : self.nx] = sfc["vdep"]
            keep["svdep"] = v
            f.vdep = v.ctypes.data
        o = FpxFieldsOut()
        res = {}
        for k in want:
            res[k] = np.zeros((self.nzmax, self.nymax, self.nxmax), rt)
            setattr(o, k, res[k].ctypes.data)
        hgt = np.zeros(self.nz, rt)
        o.height = hgt.ctypes.data
        nmixz = C.c_int32(0)
        o.nmixz = C.pointer(nmixz)
        import time as _time
        t0 = _time.perf_counter()
        check(self.lib.fpx_verttransform_ecmwf(self.h, int(slot), C.byref(ml), C.byref(f) if sfc is not None else None, C.byref(o)),
              "fpx_verttransform_ecmwf")
        call_s = _time.perf_counter() - t0          # the C call alone (the marshalling above is the mirror's, not the host's)
        out = {k: v[: self.nz, : self.ny, : self.nx].astype(np.float64) for k, v in res.items()}
        out["height"] = hgt.astype(np.float64)
        out["nmixz"] = int(nmixz.value)
        ms = C.c_double(0)
        check(self.lib.fpx_verttransform_time(self.h, C.byref(ms)), "fpx_verttransform_time")
        out["device_ms"] = ms.value
        check(self.lib.fpx_calcpv_time(self.h, C.byref(ms)), "fpx_calcpv_time")
        out["calcpv_ms"] = ms.value
        out["call_ms"] = call_s * 1e3
        return out

    def verttransform_gfs(self, slot, m, sfc, *, init=False,
                          want=("uu", "vv", "ww", "tt", "qv", "pv", "rho", "drhodz", "uupol", "vvpol", "pplev"), device_pv=False):
        """fpx_verttransform_gfs: m = synthetic.gfs_levels() dict (compact [nz][ny][nx] arrays, akz = the pressures of the
        levels), sfc = dict of compact 2-D fields (hmix, ustar, wstar, oli, tropopause[, vdep]) of this slot; sfc = None is
        passed through as NULL (the library refuses it); sfc = {} leaves the five 2-D members NULL: calcpar_gfs(slot, ..)
        follows and the slot stays "not loaded" until it has run.  device_pv: pvh = NULL, calcpv runs on the device.
        Returns the z-level arrays asked for (compact; "pplev" is the GFS extra), height and nmixz."""
        from ._lib import FpxModelLevels, FpxFieldsOut
        rt = self.hreal
        keep = {}
        ml = FpxModelLevels()
        for k in ("uuh", "vvh", "pvh", "wwh", "tth", "qvh"):
            if k == "pvh" and device_pv:
                continue
            keep[k] = np.zeros((self.nzmax, self.nymax, self.nxmax), rt)
            keep[k][: self.nz, : self.ny, : self.nx] = m[k]
            setattr(ml, k, keep[k].ctypes.data)
        for k in ("ps", "tt2", "td2"):
            keep[k] = np.zeros((self.nymax, self.nxmax), rt)
            keep[k][: self.ny, : self.nx] = m[k]
            setattr(ml, k, keep[k].ctypes.data)
        for k in ("akz", "bkz", "aknew", "bknew"):
            keep[k] = np.ascontiguousarray(np.asarray(m[k]).astype(rt))
            setattr(ml, k, keep[k].ctypes.data)
        ml.nuvz = ml.nwz = int(m.get("nuvz", self.nz))
        ml.init = int(init)
        f = FpxFields()
        if sfc is not None:
            for k in ("hmix", "ustar", "wstar", "oli", "tropopause"):
                if k not in sfc:            # a member left NULL; sfc = {}: all five NULL, calcpar_gfs(slot, ..) follows
                    continue
                a = np.zeros((self.nymax, self.nxmax), rt)
                a[: self.ny, : self.nx] = sfc[k]
                keep["s" + k] = a
                setattr(f, k, a.ctypes.data)
            if "vdep" in sfc:
                v = np.zeros((self.nspec, self.nymax, self.nxmax), rt)
                v[:, : self.ny, : self.nx] = sfc["vdep"]
                keep["svdep"] = v
                f.vdep = v.ctypes.data
        o = FpxFieldsOut()
        res = {}
        for k in want:
            res[k] = np.zeros((self.nzmax, self.nymax, self.nxmax), rt)
            if k != "pplev":
                setattr(o, k, res[k].ctypes.data)
        hgt = np.zeros(self.nz, rt)
        o.height = hgt.ctypes.data
        nmixz = C.c_int32(0)
        o.nmixz = C.pointer(nmixz)
        import time as _time
        t0 = _time.perf_counter()
        check(self.lib.fpx_verttransform_gfs(self.h, int(slot), C.byref(ml), C.byref(f) if sfc is not None else None, C.byref(o),
                                             res["pplev"].ctypes.data if "pplev" in res else None), "fpx_verttransform_gfs")
        call_s = _time.perf_counter() - t0
        out = {k: v[: self.nz, : self.ny, : self.nx].astype(np.float64) for k, v in res.items()}
        out["height"] = hgt.astype(np.float64)
        out["nmixz"] = int(nmixz.value)
        ms = C.c_double(0)
        check(self.lib.fpx_verttransform_time(self.h, C.byref(ms)), "fpx_verttransform_time")
        out["device_ms"] = ms.value
        check(self.lib.fpx_calcpv_time(self.h, C.byref(ms)), "fpx_calcpv_time")
        out["calcpv_ms"] = ms.value
        out["call_ms"] = call_s * 1e3
        return out

    def calcpv_init(self, dxn):
        """fpx_calcpv_init: dxn = com_mod's dxn(1:numbnests), for verttransform(.., nest=.., device_pv=True)."""
        from ._lib import FpxCalcpvCfg
        c = FpxCalcpvCfg()
        c.struct_bytes = C.sizeof(FpxCalcpvCfg)
        for i, v in enumerate(np.atleast_1d(np.asarray(dxn, dtype=np.float64))):
            c.dxn[i] = float(self.hreal(v))
        check(self.lib.fpx_calcpv_init(self.h, C.byref(c)), "fpx_calcpv_init")

    def get_pvh(self, nest=None, padded=False):
        """fpx_get_pvh: the model-level PV of the last transform of the mother grid (nest=None) or of nest 1, compact
        [nz][ny][nx] (padded: the whole host-shaped array as copied, strides nxmax, nymax or nxmaxn, nymaxn)."""
        if nest is None:
            shape, nx, ny, g = (self.nzmax, self.nymax, self.nxmax), self.nx, self.ny, 0
        else:
            nxn, nyn = self._nest_extent
            shape, nx, ny, g = (self.nzmax, nyn + self.nest_pad[1], nxn + self.nest_pad[0]), nxn, nyn, 1
        out = np.zeros(shape, self.hreal)
        check(self.lib.fpx_get_pvh(self.h, g, _vp(out)), "fpx_get_pvh")
        return out if padded else out[: self.nz, :ny, :nx].astype(np.float64)

    def calcpar(self, slot, cin, vdep=None, device_vdep=False):
        """fpx_calcpar after verttransform(slot, m, None): cin = synthetic.calcpar_inputs(m).  Returns the five 2-D fields
        (compact [ny][nx]) and the device time.  device_vdep: with DRYDEP no vdep is handed over; getvdep(slot, ..) follows."""
        from ._lib import FpxCalcparIn, FpxCalcparOut
        rt = self.hreal
        keep = {}
        c = FpxCalcparIn()
        for k in ("surfstr", "sshf", "excessoro"):
            a = np.zeros((self.nymax, self.nxmax), rt)
            a[: self.ny, : self.nx] = cin[k]
            keep[k] = a
            setattr(c, k, a.ctypes.data)
        for k in ("akm", "bkm"):
            keep[k] = np.ascontiguousarray(np.asarray(cin[k]).astype(rt))
            setattr(c, k, keep[k].ctypes.data)
        c.lsubgrid = int(cin["lsubgrid"])
        c.device_vdep = int(bool(device_vdep))
        if vdep is not None:
            v = np.zeros((self.nspec, self.nymax, self.nxmax), rt)
            v[:, : self.ny, : self.nx] = vdep
            keep["vdep"] = v
            c.vdep = v.ctypes.data
        o = FpxCalcparOut()
        res = {}
        for k in ("ustar", "wstar", "oli", "hmix", "tropopause"):
            res[k] = np.zeros((self.nymax, self.nxmax), rt)
            setattr(o, k, res[k].ctypes.data)
        check(self.lib.fpx_calcpar(self.h, int(slot), C.byref(c), C.byref(o)), "fpx_calcpar")
        out = {k: v[: self.ny, : self.nx].astype(np.float64) for k, v in res.items()}
        ms = C.c_double(0)
        check(self.lib.fpx_calcpar_time(self.h, C.byref(ms)), "fpx_calcpar_time")
        out["device_ms"] = ms.value
        return out

    def calcpar_gfs(self, slot, cin, vdep=None, device_vdep=False):
        """fpx_calcpar_gfs after verttransform_gfs(slot, m, {}): cin = synthetic.calcpar_gfs_inputs(m) (surfstr, sshf, excessoro,
        the GRIB file's raw hmix, lsubgrid).  Returns the five 2-D fields (compact [ny][nx]) and the device time.
        device_vdep: with DRYDEP no vdep is handed over; getvdep(slot, ..) follows."""
        from ._lib import FpxCalcparGfsIn, FpxCalcparOut
        rt = self.hreal
        keep = {}
        c = FpxCalcparGfsIn()
        c.struct_bytes = C.sizeof(FpxCalcparGfsIn)
        for k in ("surfstr", "sshf", "excessoro", "hmix"):
            if cin.get(k) is None:          # left NULL: the library says what is missing
                continue
            a = np.zeros((self.nymax, self.nxmax), rt)
            a[: self.ny, : self.nx] = cin[k]
            keep[k] = a
            setattr(c, k, a.ctypes.data)
        c.lsubgrid = int(cin["lsubgrid"])
        c.device_vdep = int(bool(device_vdep))
        if vdep is not None:
            v = np.zeros((self.nspec, self.nymax, self.nxmax), rt)
            v[:, : self.ny, : self.nx] = vdep
            keep["vdep"] = v
            c.vdep = v.ctypes.data
        o = FpxCalcparOut()
        res = {}
        for k in ("ustar", "wstar", "oli", "hmix", "tropopause"):
            res[k] = np.zeros((self.nymax, self.nxmax), rt)
            setattr(o, k, res[k].ctypes.data)
        import time as _time
        t0 = _time.perf_counter()
        check(self.lib.fpx_calcpar_gfs(self.h, int(slot), C.byref(c), C.byref(o)), "fpx_calcpar_gfs")
        call_s = _time.perf_counter() - t0
        out = {k: v[: self.ny, : self.nx].astype(np.float64) for k, v in res.items()}
        ms = C.c_double(0)
        check(self.lib.fpx_calcpar_time(self.h, C.byref(ms)), "fpx_calcpar_time")
        out["device_ms"] = ms.value
        out["call_ms"] = call_s * 1e3
        return out

    def getvdep_init(self, tables):
        """fpx_getvdep_init: tables = synthetic.getvdep_tables() (xlanduse compact [numclass][ny][nx], the small tables in
        com_mod's shapes, transposed to C order)."""
        from ._lib import FpxGetvdepTables
        rt = self.hreal
        t = FpxGetvdepTables()
        t.numclass, t.ni, t.maxspec = int(tables["numclass"]), int(tables["ni"]), int(tables["maxspec"])
        t.bdate = float(tables["bdate"])
        keep = {}
        xl = np.zeros((t.numclass, self.nymax, self.nxmax), rt)
        xl[:, : self.ny, : self.nx] = tables["xlanduse"]
        keep["xlanduse"] = xl
        for k in ("z0", "ri", "rac", "rcl", "rgs", "rlu", "rm", "reldiff", "henry", "f0", "density", "dryvel", "vset", "schmi", "fract"):
            keep[k] = np.ascontiguousarray(np.asarray(tables[k]).astype(rt))
        for k, a in keep.items():
            setattr(t, k, a.ctypes.data)
        check(self.lib.fpx_getvdep_init(self.h, C.byref(t)), "fpx_getvdep_init")

    def getvdep(self, slot, gin, *, given=None):
        """fpx_getvdep: gin = synthetic.getvdep_inputs() (wftime and compact [ny][nx] ssr, lsprec, convprec, sd); `given`: a
        dict with any of ustar, oli, ps, tt2, td2 as the host's arrays -- what is missing is taken from the device
        (fpx_calcpar, fpx_verttransform_ecmwf of this slot).  Returns vdep [nspec][ny][nx] as copied back, and the times."""
        from ._lib import FpxGetvdepIn
        import time as _time
        rt = self.hreal
        g = FpxGetvdepIn()
        g.wftime = int(gin["wftime"])
        keep = {}
        src = {k: gin[k] for k in ("ssr", "lsprec", "convprec", "sd")}
        src.update(given or {})
        for k, v in src.items():
            a = np.zeros((self.nymax, self.nxmax), rt)
            a[: self.ny, : self.nx] = v
            keep[k] = a
            setattr(g, k, a.ctypes.data)
        out = np.zeros((self.nspec, self.nymax, self.nxmax), rt)
        t0 = _time.perf_counter()
        check(self.lib.fpx_getvdep(self.h, int(slot), C.byref(g), _vp(out)), "fpx_getvdep")
        call_s = _time.perf_counter() - t0
        ms = C.c_double(0)
        check(self.lib.fpx_getvdep_time(self.h, C.byref(ms)), "fpx_getvdep_time")
        return dict(vdep=out[:, : self.ny, : self.nx].astype(np.float64), device_ms=ms.value, call_ms=call_s * 1e3)

    def _nest_compact(self, a, nest):
        nxn, nyn = self._nest_extents[nest - 1]
        return a[..., :nyn, :nxn].astype(np.float64)

    def calcpar_nest(self, nest, slot, cin, vdep=None, device_vdep=False, padded=False):
        """fpx_calcpar_nest after verttransform(slot, n, None, nest=nest): cin = synthetic.calcpar_inputs(n) of the nest (compact
        [nyn][nxn]).  Returns the five 2-D fields (compact; padded: the host-shaped arrays as copied back) and the device time."""
        from ._lib import FpxCalcparIn, FpxCalcparOut
        rt = self.hreal
        keep = {}
        c = FpxCalcparIn()
        for k in ("surfstr", "sshf", "excessoro"):
            if cin.get(k) is None:
                continue
            keep[k] = self._nest_host(cin[k])
            setattr(c, k, keep[k].ctypes.data)
        for k in ("akm", "bkm"):
            keep[k] = np.ascontiguousarray(np.asarray(cin[k]).astype(rt))
            setattr(c, k, keep[k].ctypes.data)
        c.lsubgrid = int(cin["lsubgrid"])
        c.device_vdep = int(bool(device_vdep))
        if vdep is not None:
            keep["vdep"] = self._nest_host(vdep)
            c.vdep = keep["vdep"].ctypes.data
        o = FpxCalcparOut()
        res = {}
        for k in ("ustar", "wstar", "oli", "hmix", "tropopause"):
            res[k] = np.zeros((self._nest_max[1], self._nest_max[0]), rt)
            setattr(o, k, res[k].ctypes.data)
        check(self.lib.fpx_calcpar_nest(self.h, int(nest), int(slot), C.byref(c), C.byref(o)), "fpx_calcpar_nest")
        out = res if padded else {k: self._nest_compact(v, nest) for k, v in res.items()}
        ms = C.c_double(0)
        check(self.lib.fpx_calcpar_time(self.h, C.byref(ms)), "fpx_calcpar_time")
        out["device_ms"] = ms.value
        return out

    def getvdep_nest_init(self, nest, xlanduse):
        """fpx_getvdep_nest_init: xlandusen of nest `nest`, compact [numclass][nyn][nxn]; after getvdep_init (the shared tables)."""
        xl = self._nest_host(xlanduse)
        check(self.lib.fpx_getvdep_nest_init(self.h, int(nest), _vp(xl)), "fpx_getvdep_nest_init")

    def getvdep_nest(self, nest, slot, gin, given=None):
        """fpx_getvdep_nest: gin = synthetic.getvdep_inputs() on the nest (wftime and compact [nyn][nxn] ssr, lsprec, convprec, sd);
        `given`: any of ustar, oli, ps, tt2, td2 as the host's arrays -- what is missing is taken from the device
        (fpx_calcpar_nest, fpx_verttransform_nest of this nest and slot).  Returns vdepn [nspec][nyn][nxn] as copied back, and the times."""
        from ._lib import FpxGetvdepIn
        import time as _time
        g = FpxGetvdepIn()
        g.wftime = int(gin["wftime"])
        keep = {}
        src = {k: gin[k] for k in ("ssr", "lsprec", "convprec", "sd")}
        src.update(given or {})
        for k, v in src.items():
            if v is None:
                continue
            keep[k] = self._nest_host(v)
            setattr(g, k, keep[k].ctypes.data)
        out = np.zeros((self.nspec, self._nest_max[1], self._nest_max[0]), self.hreal)
        t0 = _time.perf_counter()
        check(self.lib.fpx_getvdep_nest(self.h, int(nest), int(slot), C.byref(g), _vp(out)), "fpx_getvdep_nest")
        call_s = _time.perf_counter() - t0
        ms = C.c_double(0)
        check(self.lib.fpx_getvdep_time(self.h, C.byref(ms)), "fpx_getvdep_time")
        return dict(vdep=self._nest_compact(out, nest), device_ms=ms.value, call_ms=call_s * 1e3)

    def _verttransform_nest(self, slot, n, sfc, want, device_pv=False, nest=1):
        from ._lib import FpxModelLevels, FpxFieldsOut
        rt = self.hreal
        nxn, nyn = int(n["grid"][0]), int(n["grid"][1])
        keep = {}
        ml = FpxModelLevels()
        for k in ("uuh", "vvh", "pvh", "wwh", "tth", "qvh"):
            if k == "pvh" and device_pv:
                continue
            keep[k] = self._nest_host(n[k], nlev=self.nzmax)
            setattr(ml, k, keep[k].ctypes.data)
        for k in ("ps", "tt2", "td2"):
            keep[k] = self._nest_host(n[k])
            setattr(ml, k, keep[k].ctypes.data)
        for k in ("akz", "bkz", "aknew", "bknew"):
            keep[k] = np.ascontiguousarray(np.asarray(n[k]).astype(rt))
            setattr(ml, k, keep[k].ctypes.data)
        ml.nuvz = ml.nwz = self.nz
        ml.nest_dy, ml.nest_ylat0 = float(rt(n["geom"][1])), float(rt(n["geom"][3]))
        f = FpxFields()
        for k in ("hmix", "ustar", "wstar", "oli", "tropopause", "vdep"):
            if sfc is None or (k == "vdep" and "vdep" not in sfc):      # sfc = None: calcpar_nest(nest, slot, ..) follows
                continue
            keep["s" + k] = self._nest_host(sfc[k])
            setattr(f, k, keep["s" + k].ctypes.data)
        o = FpxFieldsOut()
        res = {}
        nxmaxn, nymaxn = self._nest_max or (nxn + self.nest_pad[0], nyn + self.nest_pad[1])
        for k in want:
            if k in ("uupol", "vvpol"):
                continue
            res[k] = np.zeros((self.nzmax, nymaxn, nxmaxn), rt)
            setattr(o, k, res[k].ctypes.data)
        check(self.lib.fpx_verttransform_nest(self.h, int(nest), int(slot), C.byref(ml), C.byref(f) if sfc is not None else None, C.byref(o)), "fpx_verttransform_nest")
        return {k: v[: self.nz, :nyn, :nxn].astype(np.float64) for k, v in res.items()}

    def upload_diag_fields_from_scenario(self, sc):
        """oro and, for both slots, pv, qv, tt (compact arrays) -> fpx_upload_diag_fields."""
        from ._lib import FpxDiagFields
        rt = self.hreal
        oro = np.zeros((self.nymax, self.nxmax), rt)
        oro[: self.ny, : self.nx] = sc["oro"]
        f = FpxDiagFields()
        f.oro = oro.ctypes.data
        check(self.lib.fpx_upload_diag_fields(self.h, 0, C.byref(f)), "fpx_upload_diag_fields")
        for m in (0, 1):
            keep = {}
            f = FpxDiagFields()
            for k in ("pv", "qv", "tt"):
                keep[k] = self._host3(sc[k], m)
                setattr(f, k, keep[k].ctypes.data)
            check(self.lib.fpx_upload_diag_fields(self.h, m + 1, C.byref(f)), "fpx_upload_diag_fields")

    def upload_diag_nest_fields(self, nest, oron, ttn2=None):
        """oron [nyn][nxn] and ttn of time slot 2 [nz][nyn][nxn] of a nested wind field (compact; padded here by nest_pad)."""
        from ._lib import FpxDiagFields
        f = FpxDiagFields()
        o = self._nest_host(oron)
        f.oro = o.ctypes.data
        t = None
        if ttn2 is not None:
            t = self._nest_host(ttn2, nlev=self.nzmax)
            f.tt = t.ctypes.data
        check(self.lib.fpx_upload_diag_nest_fields(self.h, int(nest), 2 if ttn2 is not None else 0, C.byref(f)), "fpx_upload_diag_nest_fields")

    def partoutput(self, itime, path):
        """fpx_partoutput: writes the reference's partposit_* dump to `path`; returns the number of particle records."""
        n = C.c_int64(0)
        check(self.lib.fpx_partoutput(self.h, int(itime), str(path).encode(), C.byref(n)), "fpx_partoutput")
        ms = C.c_double(0)
        check(self.lib.fpx_partoutput_time(self.h, C.byref(ms)), "fpx_partoutput_time")
        self.partoutput_device_ms = ms.value
        return int(n.value)

    def readpartpositions(self, path, jul_header, bdate, mintime, nclassunc=1, itrasplit=999999999):
        """fpx_readpartpositions: warm start from the dump `path`; -> (numpart, numparticlecount, itimein)."""
        from ._lib import FpxRestart
        r = FpxRestart(float(jul_header), float(bdate), int(mintime), int(nclassunc), int(itrasplit), 0)
        n = C.c_int64(0); npc = C.c_int32(0); it = C.c_int32(0)
        check(self.lib.fpx_readpartpositions(self.h, str(path).encode(), C.byref(r), C.byref(n), C.byref(npc), C.byref(it)),
              "fpx_readpartpositions")
        self.n = int(n.value)
        return int(n.value), int(npc.value), int(it.value)

    # ---- convective mixing (fpx_conv_init / fpx_upload_conv_fields / fpx_convmix) ----
    def conv_init(self, cs):
        """Level structure of a synthetic.convection_case()-like dict: grid[2] = nuvz, nconvlev, akz, bkz, akm, bkm."""
        from ._lib import FpxConvConfig
        rt = self.hreal
        c = FpxConvConfig()
        c.struct_bytes = C.sizeof(FpxConvConfig)
        c.nuvz, c.nconvlev = int(cs["grid"][2]), int(cs["nconvlev"])
        keep = {k: np.ascontiguousarray(np.asarray(cs[k]).astype(rt)) for k in ("akz", "bkz", "akm", "bkm")}
        for k, a in keep.items():
            setattr(c, k, a.ctypes.data)
        check(self.lib.fpx_conv_init(self.h, C.byref(c)), "fpx_conv_init")
        self.conv_nuvz, self.conv_nconvlev = c.nuvz, c.nconvlev
        self.has_conv = True

    def upload_conv_fields(self, slot, ps, tt2, td2, tth, qvh, nuvzmax=None):
        """One wind-field slot of ps, tt2, td2 [ny][nx] and tth, qvh [nuvz][ny][nx] (compact), padded to the host layout."""
        from ._lib import FpxConvFields
        rt = self.hreal
        nuvz = int(np.asarray(tth).shape[0])
        nuvzmax = nuvz + 1 if nuvzmax is None else int(nuvzmax)
        f = FpxConvFields()
        keep = {}
        for k, a in (("ps", ps), ("tt2", tt2), ("td2", td2)):
            b = np.zeros((self.nymax, self.nxmax), rt)
            b[: self.ny, : self.nx] = a
            keep[k] = b
            setattr(f, k, b.ctypes.data)
        for k, a in (("tth", tth), ("qvh", qvh)):
            b = np.zeros((nuvzmax, self.nymax, self.nxmax), rt)
            b[:nuvz, : self.ny, : self.nx] = a
            keep[k] = b
            setattr(f, k, b.ctypes.data)
        f.nuvzmax = nuvzmax
        check(self.lib.fpx_upload_conv_fields(self.h, int(slot), C.byref(f)), "fpx_upload_conv_fields")

    def upload_conv_nest_fields(self, nest, slot, ps, tt2, td2, tth, qvh, nuvzmax=None):
        """The same five arrays of nested wind field `nest` [nyn][nxn] / [nuvz][nyn][nxn] (compact; padded here by nest_pad)."""
        from ._lib import FpxConvFields
        nuvz = int(np.asarray(tth).shape[0])
        nuvzmax = nuvz + 1 if nuvzmax is None else int(nuvzmax)
        f = FpxConvFields()
        keep = {}
        for k, a in (("ps", ps), ("tt2", tt2), ("td2", td2)):
            keep[k] = self._nest_host(a)
            setattr(f, k, keep[k].ctypes.data)
        for k, a in (("tth", tth), ("qvh", qvh)):
            keep[k] = self._nest_host(a, nlev=nuvzmax)
            setattr(f, k, keep[k].ctypes.data)
        f.nuvzmax = nuvzmax
        check(self.lib.fpx_upload_conv_nest_fields(self.h, int(nest), int(slot), C.byref(f)), "fpx_upload_conv_nest_fields")

    def cbaseflux_nest(self, nest, shape, new=None):
        a = np.zeros(shape, self.hreal)
        if new is not None:
            a[:] = new
            check(self.lib.fpx_set_cbaseflux_nest(self.h, int(nest), a.ctypes.data), "fpx_set_cbaseflux_nest")
            return None
        check(self.lib.fpx_get_cbaseflux_nest(self.h, int(nest), a.ctypes.data), "fpx_get_cbaseflux_nest")
        return a.astype(np.float64)

    def convmix(self, itime=None):
        """fpx_convmix: -> number of particles whose height was set; .convmix_device_ms holds the device time."""
        n = C.c_int64(0)
        check(self.lib.fpx_convmix(self.h, int(self.itime if itime is None else itime), C.byref(n)), "fpx_convmix")
        ms = C.c_double(0)
        check(self.lib.fpx_convmix_time(self.h, C.byref(ms)), "fpx_convmix_time")
        self.convmix_device_ms = ms.value
        return int(n.value)

    def conv_columns(self, cols):
        """fpx_conv_columns: what the last convmix() left for the columns `cols` (numbered through all wind-field domains, mother
        grid first) -> lconv [n] (-1: not visited), nconvtop [n], fmassfrac [n][nconvlev+1][nconvlev+1] ((k, kk) at [kk-1][k-1]) and
        uvzlev [n][nconvlev+2] as float64, zero beyond nconvtop (nconvtop + 1).  Raises FpxError (code -3) when the call ran more
        than one matrix batch."""
        col = np.ascontiguousarray(cols, np.int32).ravel()
        n, nl = int(col.size), self.conv_nconvlev + 1
        lconv = np.zeros(n, np.int32); ntop = np.zeros(n, np.int32)
        fm = np.zeros((n, nl, nl), self.hreal); uvz = np.zeros((n, nl + 1), self.hreal)
        check(self.lib.fpx_conv_columns(self.h, col.ctypes.data, n, lconv.ctypes.data, ntop.ctypes.data, fm.ctypes.data, uvz.ctypes.data),
              "fpx_conv_columns")
        return lconv, ntop, fm.astype(np.float64), uvz.astype(np.float64)

    # ---- the NCEP GFS branch (fpx_conv_init_gfs / fpx_upload_conv_gfs_fields / fpx_conv_soundings) ----
    def conv_init_gfs(self, cs):
        """Level structure of a synthetic.convection_case_gfs()-like dict: grid[2] = nuvz (= nz of the engine), nconvlev."""
        from ._lib import FpxConvGfsConfig
        c = FpxConvGfsConfig()
        c.struct_bytes = C.sizeof(FpxConvGfsConfig)
        c.nuvz, c.nconvlev = int(cs["grid"][2]), int(cs["nconvlev"])
        check(self.lib.fpx_conv_init_gfs(self.h, C.byref(c)), "fpx_conv_init_gfs")
        self.conv_nuvz, self.conv_nconvlev = c.nuvz, c.nconvlev
        self.has_conv = True

    def upload_conv_gfs_fields(self, slot, ps, tt2, td2, tt, qv, pplev, nzmax=None):
        """One wind-field slot of ps, tt2, td2 [ny][nx] and the z-level tt, qv, pplev [nz][ny][nx] (compact), padded to the
        host layout (nxmax, nymax, nzmax)."""
        from ._lib import FpxConvGfsFields
        rt = self.hreal
        nz = int(np.asarray(tt).shape[0])
        nzmax = self.nzmax if nzmax is None else int(nzmax)
        f = FpxConvGfsFields()
        keep = {}
        for k, a in (("ps", ps), ("tt2", tt2), ("td2", td2)):
            b = np.zeros((self.nymax, self.nxmax), rt)
            b[: self.ny, : self.nx] = a
            keep[k] = b
            setattr(f, k, b.ctypes.data)
        for k, a in (("tt", tt), ("qv", qv), ("pplev", pplev)):
            b = np.zeros((max(nzmax, 1), self.nymax, self.nxmax), rt)
            b[: min(nz, nzmax), : self.ny, : self.nx] = np.asarray(a)[: min(nz, nzmax)]
            keep[k] = b
            setattr(f, k, b.ctypes.data)
        f.nzmax = nzmax
        check(self.lib.fpx_upload_conv_gfs_fields(self.h, int(slot), C.byref(f)), "fpx_upload_conv_gfs_fields")

    def conv_soundings(self, cols):
        """fpx_conv_soundings: the soundings the last convmix() left for the columns `cols` -> dict of psconv [n], pconv, dpr,
        tconv, qconv [n][nuvz-1], phconv [n][nuvz] in the host's real kind (bit for bit what the device holds); zeros for a
        column the call did not visit."""
        col = np.ascontiguousarray(cols, np.int32).ravel()
        n, nuvz = int(col.size), self.conv_nuvz
        out = {"psconv": np.zeros(n, self.hreal), "phconv": np.zeros((n, nuvz), self.hreal)}
        for k in ("pconv", "dpr", "tconv", "qconv"):
            out[k] = np.zeros((n, nuvz - 1), self.hreal)
        check(self.lib.fpx_conv_soundings(self.h, col.ctypes.data, n, *(out[k].ctypes.data for k in ("psconv", "pconv", "phconv", "dpr", "tconv", "qconv"))),
              "fpx_conv_soundings")
        return out

    def cbaseflux(self, new=None):
        a = np.zeros((self.ny, self.nx), self.hreal)
        if new is not None:
            a[:] = new
            check(self.lib.fpx_set_cbaseflux(self.h, a.ctypes.data), "fpx_set_cbaseflux")
            return None
        check(self.lib.fpx_get_cbaseflux(self.h, a.ctypes.data), "fpx_get_cbaseflux")
        return a.astype(np.float64)

    def checkpoint_write(self, path, itime=None, numparticlecount=None):
        """fpx_checkpoint_write: everything the particle loop carries (lossless, unlike partoutput)."""
        check(self.lib.fpx_checkpoint_write(self.h, str(path).encode(), int(self.itime if itime is None else itime),
                                            int(getattr(self, "numparticlecount", 0) if numparticlecount is None else numparticlecount)),
              "fpx_checkpoint_write")

    def checkpoint_read(self, path):
        """fpx_checkpoint_read: -> (itime, numpart, numparticlecount); the engine continues from there."""
        it = C.c_int32(0); n = C.c_int64(0); npc = C.c_int32(0)
        check(self.lib.fpx_checkpoint_read(self.h, str(path).encode(), C.byref(it), C.byref(n), C.byref(npc)), "fpx_checkpoint_read")
        self.n = int(n.value)
        self.itime = int(it.value)
        self.numparticlecount = int(npc.value)
        return self.itime, self.n, self.numparticlecount

    def get_flux(self, allreduce=False, clear=False):
        """fpx_get_flux: the gross mass fluxes accumulated since the last clear (device_flux = 1), in the host's real
        kind, shape (nageclass, maxpointspec_act, nspec, numzgrid, numygrid, numxgrid, 6)."""
        out = np.zeros(self.fshape, self.hreal)
        check(self.lib.fpx_get_flux(self.h, _vp(out), int(allreduce), int(clear)), "fpx_get_flux")
        return out

    def fluxoutput(self, itime, prefix, area, areaeast, areanorth, outstep, bdate, reduced=False):
        """fpx_fluxoutput: writes <prefix>grid_flux_<date><time> (fluxoutput.f90) and zeroes the device's flux;
        returns the file name."""
        from ._lib import FpxFluxout
        rt = self.hreal
        a = np.ascontiguousarray(np.asarray(area, dtype=rt))
        ae = np.ascontiguousarray(np.asarray(areaeast, dtype=rt))
        an = np.ascontiguousarray(np.asarray(areanorth, dtype=rt))
        nzg, nyg, nxg = self.fshape[3:6]
        if a.shape != (nyg, nxg) or ae.shape != (nzg, nyg, nxg) or an.shape != (nzg, nyg, nxg):
            raise ValueError("fluxoutput: area [numygrid][numxgrid], areaeast and areanorth [numzgrid][numygrid][numxgrid]")
        f = FpxFluxout(C.sizeof(FpxFluxout), 0, float(bdate), float(rt(outstep)), a.ctypes.data, ae.ctypes.data, an.ctypes.data)
        import glob
        before = set(glob.glob(str(prefix) + "grid_flux_*"))
        check(self.lib.fpx_fluxoutput(self.h, int(itime), C.byref(f), str(prefix).encode(), int(reduced)), "fpx_fluxoutput")
        new = sorted(set(glob.glob(str(prefix) + "grid_flux_*")) - before)
        return new[0] if new else None

    def calcfluxes_time(self, reset=False):
        """fpx_calcfluxes_time: (device ms of k_flux_save + k_calcfluxes since the last reset, steps that ran them)."""
        ms = C.c_double(0); n = C.c_int64(0)
        check(self.lib.fpx_calcfluxes_time(self.h, C.byref(ms), C.byref(n), int(reset)), "fpx_calcfluxes_time")
        return ms.value, int(n.value)

    def initcond_finish(self, itime=None):
        """fpx_initcond_finish: the loop of timemanager.f90:735-737 -- every particle with itra1 = itime contributes."""
        check(self.lib.fpx_initcond_finish(self.h, int(self.itime if itime is None else itime)), "fpx_initcond_finish")

    def get_initcond(self, allreduce=False, clear=False):
        """fpx_get_initcond: init_cond as summed so far (device_initcond = 1), in the host's real kind,
        shape (maxpointspec_act, nspec, numzgrid, numygrid, numxgrid)."""
        out = np.zeros(self.icshape, self.hreal)
        check(self.lib.fpx_get_initcond(self.h, _vp(out), int(allreduce), int(clear)), "fpx_get_initcond")
        return out

    def initial_cond_output(self, itime, prefix, ind_rel=0, rho_rel=None, reduced=False):
        """fpx_initial_cond_output: writes <prefix>grid_initial_<nnn> per species (initial_cond_output.f90); returns the
        file names."""
        from ._lib import FpxInitout
        rr = None if rho_rel is None else np.ascontiguousarray(np.asarray(rho_rel, dtype=self.hreal))
        if rr is not None and rr.size != self.icshape[0]:
            raise ValueError("initial_cond_output: rho_rel [maxpointspec_act]")
        o = FpxInitout(C.sizeof(FpxInitout), int(ind_rel), None if rr is None else rr.ctypes.data)
        check(self.lib.fpx_initial_cond_output(self.h, int(itime), C.byref(o), str(prefix).encode(), int(reduced)), "fpx_initial_cond_output")
        return [str(prefix) + "grid_initial_%03d" % (k + 1) for k in range(self.nspec)]

    def initcond_time(self, reset=False):
        """fpx_initcond_time: (device ms of k_initcond and k_initcond_finish since the last reset, steps that ran k_initcond)."""
        ms = C.c_double(0); n = C.c_int64(0)
        check(self.lib.fpx_initcond_time(self.h, C.byref(ms), C.byref(n), int(reset)), "fpx_initcond_time")
        return ms.value, int(n.value)

    def plumetraj_init(self, ireleasestart, ireleaseend, ncluster=5):
        """fpx_plumetraj_init: the release times of point_mod (seconds, one per release point) and par_mod's ncluster."""
        from ._lib import FpxPlumetrajCfg
        a = np.ascontiguousarray(ireleasestart, np.int32)
        b = np.ascontiguousarray(ireleaseend, np.int32)
        if a.ndim != 1 or a.shape != b.shape:
            raise ValueError("plumetraj_init: ireleasestart and ireleaseend [numpoint]")
        c = FpxPlumetrajCfg(C.sizeof(FpxPlumetrajCfg), a.size, int(ncluster), 0, a.ctypes.data, b.ctypes.data)
        check(self.lib.fpx_plumetraj_init(self.h, C.byref(c)), "fpx_plumetraj_init")
        self.pt_numpoint, self.pt_ncluster = int(a.size), int(ncluster)

    def plumetraj(self, itime=None, path=None):
        """fpx_plumetraj: `call plumetraj(itime)` on the device; with `path` the records are appended to that file.
        Returns the number of records (release points with particles)."""
        n = C.c_int32(0)
        check(self.lib.fpx_plumetraj(self.h, int(self.itime if itime is None else itime), None if path is None else str(path).encode(), C.byref(n)),
              "fpx_plumetraj")
        return int(n.value)

    def get_plumetraj(self):
        """fpx_get_plumetraj: the records of the last call as a dict of jpoint, npart, iterations [records],
        numb [records][ncluster] (int32) and values [records][14 + 5 ncluster] (the host's real kind, the order of the write
        statement plumetraj.f90:218-225 from xcenter on)."""
        nr, k = self.pt_numpoint, self.pt_ncluster
        out = dict(jpoint=np.zeros(nr, np.int32), npart=np.zeros(nr, np.int32), iterations=np.zeros(nr, np.int32),
                   numb=np.zeros((nr, k), np.int32), values=np.zeros((nr, 14 + 5 * k), self.hreal))
        check(self.lib.fpx_get_plumetraj(self.h, nr, _vp(out["jpoint"]), _vp(out["npart"]), _vp(out["iterations"]), _vp(out["numb"]),
                                         _vp(out["values"]), 14 + 5 * k), "fpx_get_plumetraj")
        used = int(np.count_nonzero(out["jpoint"]))          # jpoint is 1-based: the records the call filled
        return {key: v[:used] for key, v in out.items()}

    def plumetraj_time(self):
        """fpx_plumetraj_time: device ms of the last fpx_plumetraj."""
        ms = C.c_double(0)
        check(self.lib.fpx_plumetraj_time(self.h, C.byref(ms)), "fpx_plumetraj_time")
        return ms.value

    # ---- boundary conditions of a domain-filling run (boundcond_domainfill.f90) ----
    def _df_host(self, a, side, dtype):
        """[j][row][k] (or [row][k]) compact -> the host's declared (2, 0:nymax-1 | 0:nxmax-1, maxcolumn) in memory order."""
        a = np.asarray(a)
        nrow = self.nymax if side == "we" else self.nxmax
        out = np.zeros(((self.df_maxcolumn,) if a.ndim == 3 else ()) + (nrow, 2), dtype)
        out[tuple(slice(0, n) for n in a.shape)] = a
        return out

    def domainfill_init(self, sc, maxcolumn=None, numparticlecount=None):
        """fpx_domainfill_init from a scenario shaped like synthetic.domainfill_case(): nx_we, ny_sn, gdomainfill, nclassunc,
        itsplit, xmassperparticle and numcolumn_*, zcolumn_*, acc_mass_* as compact [j][row][k] arrays, padded here to the
        host's shapes with `maxcolumn` heights (default: the arrays' own)."""
        from ._lib import FpxDomainfillCfg
        rt = self.hreal
        self.df_maxcolumn = int(maxcolumn or np.asarray(sc["zcolumn_we"]).shape[0])
        keep = {}
        for side in ("we", "sn"):
            keep["numcolumn_" + side] = self._df_host(sc["numcolumn_" + side], side, np.int32)
            for k in ("zcolumn_", "acc_mass_"):
                keep[k + side] = self._df_host(np.asarray(sc[k + side]).astype(rt), side, rt)
        c = FpxDomainfillCfg()
        c.struct_bytes = C.sizeof(FpxDomainfillCfg)
        for k in range(2):
            c.nx_we[k], c.ny_sn[k] = int(sc["nx_we"][k]), int(sc["ny_sn"][k])
        c.gdomainfill, c.maxcolumn = int(sc.get("gdomainfill", 0)), self.df_maxcolumn
        c.nclassunc, c.itsplit, c.ipout = int(sc.get("nclassunc", 1)), int(sc.get("itsplit", 999999999)), int(sc.get("ipout_df", 0))
        c.xmassperparticle = float(rt(sc["xmassperparticle"]))
        for k, v in keep.items():
            setattr(c, k, v.ctypes.data)
        check(self.lib.fpx_domainfill_init(self.h, C.byref(c)), "fpx_domainfill_init")
        self.numparticlecount = int(sc.get("numparticlecount", 0) if numparticlecount is None else numparticlecount)

    def boundcond_domainfill(self, itime=None):
        """fpx_boundcond_domainfill: `call boundcond_domainfill(itime, loutend)` on the device; self.n (numpart) and
        self.numparticlecount follow.  Returns the statistics as a dict."""
        from ._lib import FpxDomainfillStats
        n = C.c_int64(self.n); npc = C.c_int32(self.numparticlecount); st = FpxDomainfillStats()
        check(self.lib.fpx_boundcond_domainfill(self.h, int(self.itime if itime is None else itime), C.byref(n), C.byref(npc), C.byref(st)),
              "fpx_boundcond_domainfill")
        self.n, self.numparticlecount = int(n.value), int(npc.value)
        return {k: getattr(st, k) for k, _ in FpxDomainfillStats._fields_}

    def get_domainfill_acc(self, compact=None):
        """fpx_get_domainfill_acc: (acc_mass_we, acc_mass_sn) in the host's shapes as [j][row][k]; compact = (ny, nx, heights)
        cuts them back."""
        rt = self.hreal
        we = np.zeros((self.df_maxcolumn, self.nymax, 2), rt); sn = np.zeros((self.df_maxcolumn, self.nxmax, 2), rt)
        check(self.lib.fpx_get_domainfill_acc(self.h, _vp(we), _vp(sn)), "fpx_get_domainfill_acc")
        if compact:
            we, sn = we[: compact[2], : compact[0]].copy(), sn[: compact[2], : compact[1]].copy()
        return we, sn

    def set_domainfill_acc(self, we, sn):
        rt = self.hreal
        we = self._df_host(np.asarray(we).astype(rt), "we", rt); sn = self._df_host(np.asarray(sn).astype(rt), "sn", rt)
        check(self.lib.fpx_set_domainfill_acc(self.h, _vp(we), _vp(sn)), "fpx_set_domainfill_acc")

    def boundcond_output(self, path):
        """fpx_boundcond_output: boundcond.bin (boundcond_domainfill.f90:568-572)."""
        check(self.lib.fpx_boundcond_output(self.h, str(path).encode()), "fpx_boundcond_output")

    def domainfill_time(self):
        """fpx_domainfill_time: device ms of the last fpx_boundcond_domainfill."""
        ms = C.c_double(0)
        check(self.lib.fpx_domainfill_time(self.h, C.byref(ms)), "fpx_domainfill_time")
        return ms.value

    PARTAVG_SUMS = ("cartx", "carty", "cartz", "z", "topo", "pv", "qv", "tt", "uu", "vv", "rho", "tro", "hmix", "energy")

    def get_partavg(self, first=0, count=None):
        """fpx_get_partavg: dict of npart_av (int32) and the fourteen running sums of partpos_average.f90 (PARTAVG_SUMS, the
        host's real kind) of the particles first .. first+count-1, in particle-number order (device_partavg = 1)."""
        n = self.n - first if count is None else count
        out = dict(npart_av=np.zeros(n, np.int32))
        for k in self.PARTAVG_SUMS:
            out[k] = np.zeros(n, self.hreal)
        ptrs = (C.c_void_p * 14)(*[out[k].ctypes.data for k in self.PARTAVG_SUMS])
        check(self.lib.fpx_get_partavg(self.h, int(first), int(n), _vp(out["npart_av"]), ptrs), "fpx_get_partavg")
        return out

    def partoutput_average(self, itime, prefix, bdate=None):
        """fpx_partoutput_average: writes <prefix>partposit_average_<date><time> (partoutput_average.f90) when bdate (julian
        date of the run's start) is given, else the file `prefix` itself, and zeroes the device's sums;
        returns (file name, number of valid particles)."""
        n = C.c_int64(0)
        if bdate is None:
            check(self.lib.fpx_partoutput_average(self.h, int(itime), str(prefix).encode(), C.byref(n)), "fpx_partoutput_average")
            return str(prefix), int(n.value)
        import glob
        self.set_option("bdate", repr(float(bdate)))
        before = {f: os.path.getmtime(f) for f in glob.glob(str(prefix) + "partposit_average_*")}
        check(self.lib.fpx_partoutput_average(self.h, int(itime), str(prefix).encode(), C.byref(n)), "fpx_partoutput_average")
        new = sorted(f for f in glob.glob(str(prefix) + "partposit_average_*") if f not in before)
        return (new[0] if new else None), int(n.value)

    def partavg_time(self, reset=False):
        """fpx_partavg_time: (device ms of k_partavg since the last reset, steps that ran it)."""
        ms = C.c_double(0); n = C.c_int64(0)
        check(self.lib.fpx_partavg_time(self.h, C.byref(ms), C.byref(n), int(reset)), "fpx_partavg_time")
        return ms.value, int(n.value)

    def concoutput(self, itime, prefix, area, volume, outnum, wetdep=False, drydep=False, clear=False, nest=False,
                   iout=1, prefix_pptv=None, outheight=None, outlon0=0.0, outlat0=0.0, weightmolar=(), reduced=False):
        """fpx_concoutput: writes <prefix><nnn> (the reference's grid_conc_* files) for every species."""
        from ._lib import FpxConcout
        a = np.ascontiguousarray(np.asarray(area, dtype=np.float32))
        v = np.ascontiguousarray(np.asarray(volume, dtype=np.float32))
        c = FpxConcout(a.ctypes.data, v.ctypes.data, float(outnum), int(wetdep), int(drydep), int(nest), int(iout))
        if prefix_pptv is not None:
            oh = np.ascontiguousarray(np.asarray(outheight, dtype=np.float32))
            c.prefix_pptv = str(prefix_pptv).encode(); c.outheight = oh.ctypes.data
            c.outlon0, c.outlat0 = float(outlon0), float(outlat0)
            for i, w in enumerate(weightmolar):
                c.weightmolar[i] = float(w)
        c.reduced = int(reduced)
        check(self.lib.fpx_concoutput(self.h, int(itime), C.byref(c), str(prefix).encode(), int(clear)), "fpx_concoutput")

    def upload_nests_from_scenario(self, sc):
        """One nested grid: geometry as gridcheck_nests.f90:362-378 derives it, fields uun, vvn, ..."""
        rt = self.hreal
        self.init_nest(sc["nest"], sc["nestgeom"])
        for m in (0, 1):
            self._upload_nest_slot(sc, m)

    def init_nest(self, nest, nestgeom):
        """fpx_nests_init for one nested grid: geometry as gridcheck_nests.f90:359-372 derives it."""
        self.init_nests([(nest, nestgeom)])

    def init_nests(self, nests):
        """fpx_nests_init for the nested grids [((nxn, nyn), (dxn, dyn, xlon0n, ylat0n)), ...]: geometry as
        gridcheck_nests.f90:359-372 derives it.  The host's arrays of all nests share nxmaxn, nymaxn (par_mod): the largest
        extents plus nest_pad."""
        rt = self.hreal
        dx, dy, xlon0, ylat0 = (rt(self.cfg.dx), rt(self.cfg.dy), rt(self.cfg.xlon0), rt(self.cfg.ylat0))
        n = FpxNests()
        n.struct_bytes = C.sizeof(FpxNests)
        n.numbnests = len(nests)
        self._nest_extents = [(int(e[0]), int(e[1])) for e, _ in nests]
        self._nest_extent = self._nest_extents[0]
        self._nest_max = (max(e[0] for e in self._nest_extents) + self.nest_pad[0], max(e[1] for e in self._nest_extents) + self.nest_pad[1])
        n.nxmaxn, n.nymaxn = self._nest_max
        for l, ((nxn, nyn), nestgeom) in enumerate(nests):
            nxn, nyn = int(nxn), int(nyn)
            dxn, dyn, xlon0n, ylat0n = (rt(v) for v in nestgeom)
            n.nxn[l], n.nyn[l] = nxn, nyn
            xaux2 = xlon0n + rt(nxn - 1) * dxn
            yaux2 = ylat0n + rt(nyn - 1) * dyn
            n.xresoln[l] = float(dx / dxn); n.yresoln[l] = float(dy / dyn)
            n.xln[l] = float((xlon0n - xlon0) / dx); n.xrn[l] = float((xaux2 - xlon0) / dx)
            n.yln[l] = float((ylat0n - ylat0) / dy); n.yrn[l] = float((yaux2 - ylat0) / dy)
        check(self.lib.fpx_nests_init(self.h, C.byref(n)), "fpx_nests_init")

    def _upload_nest_slot(self, sc, m):
        if True:
            keep = {}
            f = FpxFields()
            for k, kn in (("uu", "uun"), ("vv", "vvn"), ("ww", "wwn"), ("rho", "rhon"), ("drhodz", "drhodzn")):
                keep[k] = self._nest_host(np.asarray(sc[kn])[m])
                setattr(f, k, keep[k].ctypes.data)
            for k, kn in (("hmix", "hmixn"), ("ustar", "ustarn"), ("wstar", "wstarn"), ("oli", "olin"),
                          ("tropopause", "tropopausen")):
                keep[k] = self._nest_host(np.asarray(sc[kn])[m])
                setattr(f, k, keep[k].ctypes.data)
            if "vdepn" in sc:
                keep["vdep"] = self._nest_host(np.asarray(sc["vdepn"])[m])
                f.vdep = keep["vdep"].ctypes.data
            check(self.lib.fpx_upload_nest_fields(self.h, 1, m + 1, C.byref(f)), "fpx_upload_nest_fields")

    def set_release_points(self, xmass, npart):
        """point_mod xmass(numpoint,maxspec) (given as [nspec][numpoint]) and npart(numpoint)."""
        xm = np.ascontiguousarray(np.asarray(xmass, dtype=np.float64).reshape(self.nspec, -1).astype(self.hreal))
        npt = np.ascontiguousarray(np.asarray(npart, dtype=np.int32).ravel())
        assert xm.shape[1] == npt.size
        check(self.lib.fpx_set_release_points(self.h, int(npt.size), _vp(xm), npt.ctypes.data_as(C.POINTER(C.c_int32))),
              "fpx_set_release_points")
        self.numpoint = int(npt.size)

    # ---- releaseparticles + splitting on the device ------------------------------------------------------
    def release_init(self, rs):
        """fpx_release_init from a release scenario dict (synthetic.release_case): the point_mod / com_mod tables."""
        from ._lib import FpxRelease
        rt = self.hreal
        nsp, np_ = self.nspec, int(rs["numpoint"])
        self.set_release_points(np.asarray(rs["xmass"]).reshape(nsp, np_), rs["npart_rel"])
        keep = {}
        r = FpxRelease()
        r.struct_bytes = C.sizeof(FpxRelease)
        r.numpoint = np_
        for k in ("ireleasestart", "ireleaseend"):
            keep[k] = np.ascontiguousarray(np.asarray(rs[k], dtype=np.int32)); setattr(r, k, keep[k].ctypes.data)
        keep["kindz"] = np.ascontiguousarray(np.asarray(rs["kindz"], dtype=np.int16)); r.kindz = keep["kindz"].ctypes.data
        for k in ("xpoint1", "xpoint2", "ypoint1", "ypoint2", "zpoint1", "zpoint2"):
            keep[k] = np.ascontiguousarray(np.asarray(rs[k]).astype(rt)); setattr(r, k, keep[k].ctypes.data)
        for k, n2 in (("point_hour", 24), ("area_hour", 24), ("point_dow", 7), ("area_dow", 7)):
            if k in rs:       # given compact [n2][nspec]; the host arrays are (maxspec, n2) column-major with maxspec = nspec here
                keep[k] = np.ascontiguousarray(np.asarray(rs[k]).reshape(n2, nsp).astype(rt)); setattr(r, k, keep[k].ctypes.data)
        r.bdate = float(rs["bdate_jul"])
        sw = [int(v) for v in rs["switches"]]
        r.itsplit, r.ind_rel, r.nclassunc = sw[3], sw[4], int(rs.get("nclassunc", 1))
        check(self.lib.fpx_release_init(self.h, C.byref(r)), "fpx_release_init")
        self.xmasssave = np.zeros(np_, rt)
        self.rho_rel = np.zeros(np_, rt)
        self.numparticlecount = 0

    def releaseparticles(self, itime):
        """fpx_releaseparticles; returns the number of particles released; self.n (numpart) follows."""
        n = C.c_int64(self.n); npc = C.c_int32(self.numparticlecount); nrel = C.c_int64(0)
        check(self.lib.fpx_releaseparticles(self.h, int(itime), C.byref(n), C.byref(npc), _vp(self.xmasssave), _vp(self.rho_rel),
                                            C.byref(nrel)), "fpx_releaseparticles")
        self.n, self.numparticlecount = int(n.value), int(npc.value)
        return int(nrel.value)

    def split_particles(self, itime):
        n = C.c_int64(self.n)
        check(self.lib.fpx_split_particles(self.h, int(itime), C.byref(n)), "fpx_split_particles")
        self.n = int(n.value)

    def set_numpart(self, n):
        """numpart (com_mod.f90:676) as the host sees it; a smaller value than the engine's puts a locality-sorted cloud back
        into particle-number order first (the spaces beyond numpart must be vacant)."""
        check(self.lib.fpx_set_numpart(self.h, int(n)), "fpx_set_numpart")
        self.n = int(n)

    # ---- mpi_mod.f90:566-856: levelling the ranks' particle counts (the host keeps the transport) ----
    def redist_pack(self, itime, num_trans):
        """Sender: the last num_trans storage spaces -> one message (numpy uint8 array); they are terminated, self.n shrinks."""
        nb = int(self.lib.fpx_redist_bytes(self.h, int(num_trans)))
        buf = np.zeros(max(nb, 1), np.uint8)
        n = C.c_int64(self.n)
        check(self.lib.fpx_redist_pack(self.h, int(itime), int(num_trans), _vp(buf), nb, C.byref(n)), "fpx_redist_pack")
        self.n = int(n.value)
        return buf[:nb]

    def redist_unpack(self, itime, num_trans, buf):
        """Receiver: places the message's particles that are alive at itime into vacant storage spaces; self.n follows."""
        buf = np.ascontiguousarray(buf, np.uint8)
        n = C.c_int64(self.n)
        check(self.lib.fpx_redist_unpack(self.h, int(itime), int(num_trans), _vp(buf), buf.size, C.byref(n)), "fpx_redist_unpack")
        self.n = int(n.value)

    def set_windtime(self, memtime, memind):
        mt = (C.c_int32 * 2)(int(memtime[0]), int(memtime[1]))
        mi = (C.c_int32 * 2)(int(memind[0]), int(memind[1]))
        check(self.lib.fpx_set_windtime(self.h, mt, mi), "fpx_set_windtime")

    # ---- particles ----------------------------------------------------------
    def upload_particles_from_scenario(self, sc, first=0):
        n = int(sc["npart"])
        rt = self.hreal
        keep = {}
        p = FpxParticles()

        def put(name, key, dtype):
            if key in sc:
                keep[name] = np.ascontiguousarray(np.asarray(sc[key]).astype(dtype))
                setattr(p, name, keep[name].ctypes.data)
        put("xtra1", "xtra1", np.float64); put("ytra1", "ytra1", np.float64); put("ztra1", "ztra1", rt)
        for k in ("uap", "ucp", "uzp", "us", "vs", "ws"):
            put(k, k, rt)
        for k in ("itra1", "itramem", "idt", "npoint", "nclass", "itrasplit"):
            put(k, k, np.int32)
        put("cbt", "cbt", np.int16)
        if "xmass1" in sc:
            keep["xmass1"] = np.ascontiguousarray(np.asarray(sc["xmass1"]).astype(rt).reshape(self.nspec, n))
            p.xmass1 = keep["xmass1"].ctypes.data
            p.xmass1_ld = n
        if "xscav_frac1" in sc:
            keep["xscav_frac1"] = np.ascontiguousarray(np.asarray(sc["xscav_frac1"]).astype(rt).reshape(self.nspec, n))
            p.xscav_frac1 = keep["xscav_frac1"].ctypes.data
            p.xmass1_ld = n
        check(self.lib.fpx_upload_particles(self.h, first, n, C.byref(p)), "fpx_upload_particles")
        self.n = max(self.n, first + n)

    def seed_particles(self, n, seed=0x5EED, frac_pbl=0.5, zmax=12000.0, lat_margin_cells=None, itime0=0):
        if lat_margin_cells is None:
            lat_margin_cells = 0.03 * (self.ny - 1)
        check(self.lib.fpx_seed_particles(self.h, n, seed, frac_pbl, zmax, lat_margin_cells, itime0),
              "fpx_seed_particles")
        self.n = n

    def download(self, first=0, count=None):
        n = self.n - first if count is None else count
        rt = self.hreal
        out = dict(xtra1=np.empty(n, np.float64), ytra1=np.empty(n, np.float64), ztra1=np.empty(n, rt),
                   uap=np.empty(n, rt), ucp=np.empty(n, rt), uzp=np.empty(n, rt), us=np.empty(n, rt),
                   vs=np.empty(n, rt), ws=np.empty(n, rt), itra1=np.empty(n, np.int32),
                   itramem=np.empty(n, np.int32), idt=np.empty(n, np.int32), npoint=np.empty(n, np.int32),
                   nclass=np.empty(n, np.int32), itrasplit=np.empty(n, np.int32), cbt=np.empty(n, np.int16),
                   xmass1=np.empty((self.nspec, n), rt))
        if self.bkdep:
            out["xscav_frac1"] = np.empty((self.nspec, n), rt)
        p = FpxParticles()
        for k, a in out.items():
            setattr(p, k, a.ctypes.data)
        p.xmass1_ld = n
        check(self.lib.fpx_download_particles(self.h, first, n, C.byref(p)), "fpx_download_particles")
        res = {k: (v.astype(np.float64) if v.dtype.kind == "f" else v.astype(np.int32)) for k, v in out.items()}
        return res

    # ---- output grids ---------------------------------------------------------
    def outgrid_from_scenario(self, sc):
        """OUTGRID state as readoutgrid.f90 / outgrid_init.f90 leave it."""
        rt = self.hreal
        nxg, nyg, nzg = (int(v) for v in sc["outgrid"])
        dxo, dyo, lon0, lat0 = (float(v) for v in sc["outgeom"])
        g = FpxOutgrid()
        g.struct_bytes = C.sizeof(FpxOutgrid)
        g.numxgrid, g.numygrid, g.numzgrid = nxg, nyg, nzg
        g.dxout, g.dyout = float(rt(dxo)), float(rt(dyo))
        # xoutshift=xlon0-outlon0 in the host's real kind (readoutgrid.f90:199-200)
        g.xoutshift = float(rt(self.cfg.xlon0) - rt(lon0))
        g.youtshift = float(rt(self.cfg.ylat0) - rt(lat0))
        lage = np.asarray(sc["lage"]).ravel()
        iofr = int(np.asarray(sc["concflags"]).ravel()[1])
        mps = int(sc.get("numpoint", 1)) if iofr == 1 else 1      # maxpointspec_act, readreleases.f90 / outgrid_init.f90
        ncu = int(sc.get("nclassunc", 1))
        g.maxpointspec_act, g.nclassunc = mps, ncu
        g.nageclass = len(lage)
        for i, v in enumerate(lage):
            g.lage[i] = int(v)
        g.ind_samp, g.ioutputforeachrelease = (int(v) for v in sc["concflags"])
        g.lusekerneloutput = int(sc.get("lusekerneloutput", 1))   # par_mod.f90:39 (a compile-time switch of the host)
        oh = np.ascontiguousarray(np.asarray(sc["outheight"]).astype(rt))
        check(self.lib.fpx_outgrid_init(self.h, C.byref(g), _vp(oh)), "fpx_outgrid_init")
        if "outtimes" in sc:
            check(self.lib.fpx_set_output_times(self.h, int(sc["outtimes"][0]), int(sc["outtimes"][1])),
                  "fpx_set_output_times")
        self.gshape = (len(lage), ncu, mps, self.nspec, nzg, nyg, nxg)
        self.fshape = (len(lage), mps, self.nspec, nzg, nyg, nxg, 6)      # flux_mod's flux, first index fastest
        self.icshape = (mps, self.nspec, nzg, nyg, nxg)                   # unc_mod's init_cond, first index fastest
        if "outgridn" in sc:          # OUTGRID_NEST (readoutgrid_nest.f90)
            nxn, nyn = (int(v) for v in sc["outgridn"])
            dxn, dyn, lon0n, lat0n = (float(v) for v in sc["outgeomn"])
            gn = FpxOutgridNest()
            gn.struct_bytes = C.sizeof(FpxOutgridNest)
            gn.numxgridn, gn.numygridn = nxn, nyn
            gn.dxoutn, gn.dyoutn = float(rt(dxn)), float(rt(dyn))
            gn.xoutshiftn = float(rt(self.cfg.xlon0) - rt(lon0n))
            gn.youtshiftn = float(rt(self.cfg.ylat0) - rt(lat0n))
            check(self.lib.fpx_outgrid_nest_init(self.h, C.byref(gn)), "fpx_outgrid_nest_init")
            self.gshape_nest = (len(lage), ncu, mps, self.nspec, nzg, nyn, nxn)
        self.nreceptor = 0
        if "receptors" in sc:         # RECEPTORS (readreceptors.f90): x, y in grid coordinates, cell area
            r = np.asarray(sc["receptors"], dtype=np.float64).reshape(3, -1)
            self.nreceptor = r.shape[1]
            rx, ry, ra = (np.ascontiguousarray(r[k].astype(rt)) for k in range(3))
            check(self.lib.fpx_receptors_init(self.h, self.nreceptor, _vp(rx), _vp(ry), _vp(ra)), "fpx_receptors_init")

    def wet_from_scenario(self, sc):
        """Wet-scavenging species parameters (readspecies.f90) + precipitation/cloud fields."""
        w = FpxWetConfig()
        w.struct_bytes = C.sizeof(FpxWetConfig)
        for i in range(self.nspec):
            w.wetdepspec[i] = int(np.asarray(sc["wetdepspec"]).ravel()[i])
            for k in ("weta_gas", "wetb_gas", "crain_aero", "csnow_aero", "ccn_aero", "in_aero", "henry"):
                getattr(w, k)[i] = float(np.asarray(sc[k]).ravel()[i])
        w.readclouds = 0
        check(self.lib.fpx_wet_init(self.h, C.byref(w)), "fpx_wet_init")
        for m in (0, 1):
            keep = {}
            f = FpxWetFields()
            for k in ("lsprec", "convprec", "tcc"):
                keep[k] = self._host2(sc[k], m)
                setattr(f, k, keep[k].ctypes.data)
            keep["tt"] = self._host3(sc["tt"], m)
            f.tt = keep["tt"].ctypes.data
            c8 = np.zeros((self.nzmax, self.nymax, self.nxmax), np.int8)
            c8[: self.nz, : self.ny, : self.nx] = np.asarray(sc["clouds"])[m]
            keep["clouds"] = c8
            f.clouds = c8.ctypes.data
            ch = np.zeros((self.nymax, self.nxmax), np.int32)
            ch[: self.ny, : self.nx] = np.asarray(sc["cloudsh"])[m]
            keep["cloudsh"] = ch
            f.cloudsh = ch.ctypes.data
            check(self.lib.fpx_upload_wet_fields(self.h, m + 1, C.byref(f)), "fpx_upload_wet_fields")
        if "lsprecn" in sc:      # the nest's own fields (nxmaxn, nymaxn as in init_nest)
            for m in (0, 1):
                keep = {}
                f = FpxWetFields()
                for k, kn in (("lsprec", "lsprecn"), ("convprec", "convprecn"), ("tcc", "tccn"), ("tt", "ttn")):
                    keep[k] = self._nest_host(np.asarray(sc[kn])[m], nlev=self.nzmax if kn == "ttn" else None)
                    setattr(f, k, keep[k].ctypes.data)
                keep["clouds"] = self._nest_host(np.asarray(sc["cloudsn"])[m], np.int8, nlev=self.nzmax)
                f.clouds = keep["clouds"].ctypes.data
                check(self.lib.fpx_upload_wet_nest_fields(self.h, 1, m + 1, C.byref(f), 0), "fpx_upload_wet_nest_fields")

    def wetdepo(self, itime=None, ltsample=None, loutnext=None):
        itime = self.itime if itime is None else itime
        ltsample = self.lsynctime if ltsample is None else ltsample
        if loutnext is None:
            loutnext = int(self.sc["outtimes"][0]) if "outtimes" in self.sc else 0
        check(self.lib.fpx_wetdepo(self.h, int(itime), int(ltsample), int(loutnext)), "fpx_wetdepo")

    # ---- OH chemistry (gethourlyOH.f90, ohreaction.f90) -------------------------
    def oh_init(self, c, struct_bytes=None):
        """fpx_oh_init from the oh_mod arrays of a case (flexpart_amd.synthetic.oh_case): lonOH, latOH, altOH, OH_field
        [12][nzOH][nyOH][nxOH], jrate_average [12][180][360], lonjr, latjr, bdate, ohcconst, ohdconst, ohnconst."""
        from ._lib import FpxOhConfig
        rt = self.hreal
        keep = {k: np.ascontiguousarray(np.asarray(c[k]).astype(rt)) for k in ("lonOH", "latOH", "altOH", "OH_field", "jrate_average", "lonjr", "latjr")}
        o = FpxOhConfig()
        o.struct_bytes = C.sizeof(FpxOhConfig) if struct_bytes is None else int(struct_bytes)
        o.nxOH, o.nyOH, o.nzOH = keep["lonOH"].size, keep["latOH"].size, keep["altOH"].size
        assert keep["OH_field"].size == 12 * o.nxOH * o.nyOH * o.nzOH and keep["jrate_average"].size == 12 * 180 * 360
        for k, a in keep.items():
            setattr(o, k, a.ctypes.data)
        o.bdate = float(c["bdate"])
        for i in range(self.nspec):
            o.ohcconst[i], o.ohdconst[i], o.ohnconst[i] = float(c["ohcconst"][i]), float(c["ohdconst"][i]), float(c["ohnconst"][i])
        check(self.lib.fpx_oh_init(self.h, C.byref(o)), "fpx_oh_init")
        self._oh_shape = (2, o.nzOH, o.nyOH, o.nxOH)

    def upload_tt(self, tt, slots=(1, 2)):
        """tt [2][nz][ny][nx] (compact) of the given time slots -> fpx_upload_diag_fields with tt alone (what fpx_ohreaction reads)."""
        from ._lib import FpxDiagFields
        for m in slots:
            f = FpxDiagFields()
            t = self._host3(np.asarray(tt), m - 1)
            f.tt = t.ctypes.data
            check(self.lib.fpx_upload_diag_fields(self.h, int(m), C.byref(f)), "fpx_upload_diag_fields")

    def gethourlyOH(self, itime=None):
        """call gethourlyOH(itime), timemanager.f90:212-216 -> the branch taken (0 nothing, 1 advanced, 2 both fields computed)."""
        check(self.lib.fpx_gethourlyOH(self.h, self.itime if itime is None else int(itime)), "fpx_gethourlyOH")
        return self.info("oh_branch")

    def ohreaction(self, itime=None, ltsample=None, loutnext=0):
        """call ohreaction(itime, lsynctime, loutnext), timemanager.f90:171-172."""
        check(self.lib.fpx_ohreaction(self.h, self.itime if itime is None else int(itime),
                                      self.lsynctime if ltsample is None else int(ltsample), int(loutnext)), "fpx_ohreaction")

    def get_oh_hourly(self):
        """(OH_hourly [2][nzOH][nyOH][nxOH], memOHtime [2]) in the host's real kind."""
        f, t = np.empty(self._oh_shape, self.hreal), np.empty(2, self.hreal)
        check(self.lib.fpx_get_oh_hourly(self.h, _vp(f), _vp(t)), "fpx_get_oh_hourly")
        return f, t

    def set_oh_hourly(self, oh_hourly, memohtime):
        f = np.ascontiguousarray(np.asarray(oh_hourly).astype(self.hreal))
        t = np.ascontiguousarray(np.asarray(memohtime).astype(self.hreal))
        assert f.shape == self._oh_shape and t.size == 2
        check(self.lib.fpx_set_oh_hourly(self.h, _vp(f), _vp(t)), "fpx_set_oh_hourly")

    def ohreaction_time(self):
        """Device time (ms) of k_oh_blend + k_ohreaction of the last ohreaction()."""
        ms = C.c_double()
        check(self.lib.fpx_ohreaction_time(self.h, C.byref(ms)), "fpx_ohreaction_time")
        return ms.value

    def wetgrid(self, allreduce=False):
        na, nc, mp, nsp, nzg, nyg, nxg = self.gshape
        d = np.empty((na, nc, mp, nsp, nyg, nxg), np.float32)
        check(self.lib.fpx_get_wetgrid(self.h, _vp(d), int(allreduce)), "fpx_get_wetgrid")
        return d.astype(np.float64)

    def conccalc(self, itime=None, weight=1.0):
        check(self.lib.fpx_conccalc(self.h, int(self.itime if itime is None else itime), float(weight)),
              "fpx_conccalc")

    def grids(self, allreduce=False, clear=False):
        """-> (gridunc, drygridunc) as float64 arrays shaped (age, class, pointspec, spec, z, y, x) /
        (age, class, pointspec, spec, y, x)."""
        na, nc, mp, nsp, nzg, nyg, nxg = self.gshape
        g = np.empty((na, nc, mp, nsp, nzg, nyg, nxg), self.hreal)
        d = np.empty((na, nc, mp, nsp, nyg, nxg), np.float32)
        check(self.lib.fpx_get_grids(self.h, _vp(g), _vp(d), int(allreduce), int(clear)), "fpx_get_grids")
        return g.astype(np.float64), d.astype(np.float64)

    def grids_nest(self, allreduce=False, clear=False):
        """-> (griduncn, drygriduncn, wetgriduncn) of the nested output grid, float64."""
        na, nc, mp, nsp, nzg, nyg, nxg = self.gshape_nest
        g = np.empty((na, nc, mp, nsp, nzg, nyg, nxg), self.hreal)
        d = np.empty((na, nc, mp, nsp, nyg, nxg), np.float32)
        w = np.empty((na, nc, mp, nsp, nyg, nxg), np.float32)
        check(self.lib.fpx_get_grids_nest(self.h, _vp(g), _vp(d), _vp(w), int(allreduce), int(clear)), "fpx_get_grids_nest")
        return g.astype(np.float64), d.astype(np.float64), w.astype(np.float64)

    def receptors(self, allreduce=False, clear=False, ld=20):
        """-> creceptor as float64 (spec, receptor); the host array is creceptor(ld=maxreceptor, maxspec)."""
        ld = max(ld, self.nreceptor)
        c = np.zeros((self.nspec, ld), self.hreal)
        check(self.lib.fpx_get_receptors(self.h, _vp(c), ld, int(allreduce), int(clear)), "fpx_get_receptors")
        return c[:, :self.nreceptor].astype(np.float64)

    def comm_unique_id(self):
        buf = (C.c_char * 128)()
        check(self.lib.fpx_comm_unique_id(buf, 128), "fpx_comm_unique_id")
        return bytes(buf)

    def comm_init_host(self, dist, nranks, rank):
        """fpx_comm_init_host with a torch.distributed process group as the transport (what an MPI host does with
        MPI_Allreduce): the engine hands host buffers to the callback, which sums them over the ranks."""
        import torch

        def _allreduce(user, send, recv, count, dtype):
            try:
                ct = C.c_double if dtype == 1 else C.c_float
                a = np.ctypeslib.as_array(C.cast(send, C.POINTER(ct)), shape=(count,))
                t = torch.from_numpy(np.array(a, copy=True))
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                np.ctypeslib.as_array(C.cast(recv, C.POINTER(ct)), shape=(count,))[:] = t.numpy()
                return 0
            except Exception:      # never let an exception cross the C boundary
                return 1
        self._allreduce_cb = _lib.ALLREDUCE_FN(_allreduce)      # keep the thunk alive as long as the engine
        check(self.lib.fpx_comm_init_host(self.h, int(nranks), int(rank), self._allreduce_cb, None), "fpx_comm_init_host")

    def count_particles(self, allreduce=False):
        """(live, numpart) of this rank and summed over the ranks: the particle count the reference's root reduces at
        every output time (timemanager_mpi.f90:552-562)."""
        loc = (C.c_int64 * 2)()
        tot = (C.c_int64 * 2)()
        check(self.lib.fpx_count_particles(self.h, loc, tot, int(allreduce)), "fpx_count_particles")
        return (int(loc[0]), int(loc[1])), (int(tot[0]), int(tot[1]))

    def set_option(self, name, value):
        """fpx_set_option: a tuning / diagnostic knob of this handle (include/flexpart_amd.h lists the names)."""
        check(self.lib.fpx_set_option(self.h, str(name).encode(), str(value).encode()), f"fpx_set_option({name})")

    def info(self, name):
        """fpx_get_info: what the engine decided or did ("time_blended_packs", "blended_steps", "pbl_launches_per_step", ...)."""
        v = C.c_int64(0)
        check(self.lib.fpx_get_info(self.h, str(name).encode(), C.byref(v)), f"fpx_get_info({name})")
        return int(v.value)

    def lane_stats(self, reset=False):
        """Per code region of the Langevin kernel: (executions by a wave, mean active lanes); zeros unless the library was
        built with -DFPX_LANE_STATS."""
        out = (C.c_uint64 * 32)()
        check(self.lib.fpx_lane_stats(self.h, out, 32, int(reset)), "fpx_lane_stats")
        names = ("pass", "substep", "cbl", "gauss_cblflag", "exp_form", "hs_neutral", "hs_unstable", "hs_stable", "refill", "handover", "outer_loop")
        d = {nm: (int(out[2 * i]), (out[2 * i + 1] / out[2 * i]) if out[2 * i] else 0.0) for i, nm in enumerate(names)}
        nw = int(out[22])
        if nw:   # timeline of the persistent waves, all launches together (100 MHz ticks -> ms)
            ms = 1e-5
            d["timeline_ms"] = (nw, {"mean_start_to_list_exhausted": out[23] / nw * ms, "mean_start_to_end": out[24] / nw * ms,
                                     "longest_wave": out[25] * ms, "first_exhaustion": ((~out[26]) & (2**64 - 1)) * ms,
                                     "longest_drain": out[27] * ms})
        return d

    def comm_init(self, uid, nranks, rank):
        buf = (C.c_char * 128).from_buffer_copy(uid)
        check(self.lib.fpx_comm_init(self.h, buf, 128, int(nranks), int(rank)), "fpx_comm_init")

    # ---- the loop body --------------------------------------------------------
    def step(self, itime=None):
        """One pass of the particle loop at `itime` (default: the engine's clock)."""
        if itime is None:
            itime = self.itime
        st = FpxStepStats()
        check(self.lib.fpx_step(self.h, int(itime), C.byref(st)), "fpx_step")
        self.itime = int(itime) + self.lsynctime
        return {k: getattr(st, k) for k, _ in FpxStepStats._fields_}

    def step_async(self, itime=None):
        if itime is None:
            itime = self.itime
        check(self.lib.fpx_step_async(self.h, int(itime)), "fpx_step_async")
        self.itime = int(itime) + self.lsynctime

    def sync(self):
        check(self.lib.fpx_sync(self.h), "fpx_sync")

    def counters(self, reset=False):
        st = FpxStepStats()
        check(self.lib.fpx_counters(self.h, C.byref(st), int(reset)), "fpx_counters")
        return {k: getattr(st, k) for k, _ in FpxStepStats._fields_}

    def kernel_time(self, reset=False):
        ms = C.c_double(0)
        ln = C.c_int64(0)
        check(self.lib.fpx_kernel_time(self.h, C.byref(ms), C.byref(ln), int(reset)), "fpx_kernel_time")
        return ms.value, ln.value

    def kernel_times(self, reset=False):
        """(k_prep + work-list sort, k_pbl_loop, k_pbl_finish, k_prep alone) cumulative device ms and the number of steps."""
        ms = (C.c_double * 4)()
        ln = C.c_int64(0)
        check(self.lib.fpx_kernel_times(self.h, ms, C.byref(ln), int(reset)), "fpx_kernel_times")
        return list(ms), ln.value

    def sort(self):
        check(self.lib.fpx_sort_particles(self.h), "fpx_sort_particles")

    def rannumb(self):
        a = np.empty(1000000, self.hreal)
        check(self.lib.fpx_rng_get_table(self.h, _vp(a), 1000000), "fpx_rng_get_table")
        return a

    def run(self, nsteps=None):
        out = []
        for _ in range(int(self.sc["nsteps"]) if nsteps is None else nsteps):
            if self.has_wet and self.itime != 0:     # wetdepo first, timemanager.f90:164-169
                self.wetdepo()
            if self.has_conv:                        # timemanager.f90:258-262 (lconvection = 1)
                self.convmix(self.itime)
            self.step()
            if self.gshape is not None:
                self.conccalc(self.itime, 1.0)     # sample at the new positions (conccalc.f90)
            out.append(self.download())
        return out

    def close(self):
        if self.h:
            self.lib.fpx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["Engine", "RNG_TABLE_SEQ", "RNG_TABLE_COUNTER", "RNG_PHILOX"]
