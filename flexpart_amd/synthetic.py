"""Deterministic synthetic scenarios for the particle-advection path.

Everything here is built from integer arithmetic plus IEEE-exact float64
operations (+ - * / sqrt, comparisons) only -- no libm transcendentals -- so a
scenario regenerates bit-identically on any box (the GPU box has no access to
the reference tree or to scenario files made elsewhere).

A scenario is a plain dict whose keys follow the reference's own variable names
(com_mod.f90 / par_mod.f90 of the reference); see `Scenario keys` below.  Field
arrays are float64, C-ordered with shape (2, nz, ny, nx) (time slot, level, y,
x), i.e. the reference's column-major (x, y, z, slot) order with only the used
nx*ny*nz extent kept.

The shapes follow SURVEY.md section 8(d): ECMWF-like 361x181x138 global grid,
two wind-field time slots 10800 s apart, lsynctime 900 s.
"""
from __future__ import annotations

import numpy as np

# constants of the reference (par_mod.f90:59-60,76-79,112,123,213,254)
PI_REF = 3.14159265
R_EARTH = 6.371e6
HMIXMIN, HMIXMAX = 100.0, 4500.0
SWITCHNORTH, SWITCHSOUTH = 75.0, -75.0
MAXRAND = 1000000
MINSTEP = 1
DEAD = -999999999


def derive_switches(ctl_cmd: float, ifine_cmd: int, cblflag: int, lsynctime: int):
    """COMMAND-file values -> the run-time switches the hot path reads.

    Mirrors readcommand.f90:244-272,379-385 of the reference: returns a dict
    with method, mintime, turbswitch, ifine, ctl (already inverted), lsynctime.
    """
    ifine = max(int(ifine_cmd), 1)
    ctl = float(ctl_cmd)
    if cblflag == 1:
        turbswitch = True
        lsynctime = min(lsynctime, 1200)           # maxtl, com_mod.f90:752
        if ctl < 5:
            ctl = 5.0
        if ifine * ctl < 50:
            ifine = int(50.0 / ctl) + 1
    else:
        if ctl >= 0.1:
            turbswitch = True
        else:
            turbswitch = False
            ifine = 1
    ctl_inv = 1.0 / ctl
    if ctl_inv > 0.0:
        method, mintime = 1, MINSTEP
    else:
        method, mintime = 0, lsynctime
    return dict(method=method, mintime=mintime, turbswitch=int(turbswitch),
                ifine=ifine, ctl=ctl_inv, lsynctime=lsynctime, cblflag=int(cblflag))


# --------------------------------------------------------------------------
# exact building blocks
# --------------------------------------------------------------------------
def _wave(num, den):
    """C1 'parabola sine' of phase num/den (integer arrays), range [-1, 1]."""
    t = (np.asarray(num, dtype=np.int64) % int(den)).astype(np.float64) / float(den)
    return np.where(t < 0.5, 16.0 * t * (0.5 - t), -16.0 * (t - 0.5) * (1.0 - t))


def _splitmix64(n, seed):
    """n uint64 values from SplitMix64 counters (vectorised, wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(seed))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _uniform01(n, seed):
    """float64 in [0, 1) with 53 random bits, exact on every platform."""
    return (_splitmix64(n, seed) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def make_height(nz, top=80000.0, lin=0.05):
    """Stretched model-level heights [m], height[0] = 0 (verttransform output shape)."""
    s = np.arange(nz, dtype=np.float64) / float(nz - 1)
    return top * (lin * s + (1.0 - lin) * s * s * s)


def nmixz_from_height(height):
    """First level (1-based) above hmixmax, as verttransform_ecmwf.f90:186-192."""
    for kz in range(len(height)):
        if height[kz] > HMIXMAX:
            return kz + 1
    return len(height)


# --------------------------------------------------------------------------
# fields
# --------------------------------------------------------------------------
def make_fields(nx, ny, nz, height, *, uniform=None, polar=False, nspec=1, hmix_const=None):
    """Smooth synthetic met fields on an (nx, ny, nz) grid with 2 time slots.

    uniform: None for the ECMWF-shaped analytic fields, or a dict
    {u, v, w, rho, hmix, ustar, wstar, oli} for spatially uniform fields (the
    reference's own validation scenario, mpi_mod.f90:2903-2975).
    """
    f = {}
    shp3 = (2, nz, ny, nx)
    shp2 = (2, ny, nx)
    if uniform is not None:
        f["uu"] = np.full(shp3, float(uniform.get("u", 10.0)))
        f["vv"] = np.full(shp3, float(uniform.get("v", 0.0)))
        f["ww"] = np.full(shp3, float(uniform.get("w", 0.0)))
        f["rho"] = np.full(shp3, float(uniform.get("rho", 1.3)))
        f["drhodz"] = np.full(shp3, float(uniform.get("drhodz", 0.0)))
        f["tt"] = np.full(shp3, float(uniform.get("tt", 273.0)))
        f["hmix"] = np.full(shp2, float(uniform.get("hmix", 10000.0)))
        f["ustar"] = np.full(shp2, float(uniform.get("ustar", 1.0)))
        f["wstar"] = np.full(shp2, float(uniform.get("wstar", 1.0)))
        f["oli"] = np.full(shp2, float(uniform.get("oli", 0.01)))
        f["tropopause"] = np.full(shp2, float(uniform.get("tropopause", 10000.0)))
        f["vdep"] = np.full((2, nspec, ny, nx), float(uniform.get("vdep", 0.002)))
        if polar:
            f["uupol"] = f["uu"].copy()
            f["vvpol"] = f["vv"].copy()
        return f

    per = nx - 1                                   # cyclic period in x (column nx-1 == column 0)
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    s = np.arange(ny, dtype=np.float64)[None, :, None] / float(ny - 1)
    clat = 4.0 * s * (1.0 - s)                     # 0 at the poles, 1 at the equator
    z = np.asarray(height, dtype=np.float64)[:, None, None]
    zf = z / float(height[-1])
    a = z / 8000.0
    den = 1.0 + a + 0.5 * a * a
    f["uu"] = np.empty(shp3); f["vv"] = np.empty(shp3); f["ww"] = np.empty(shp3)
    f["rho"] = np.empty(shp3); f["drhodz"] = np.empty(shp3); f["tt"] = np.empty(shp3)
    for m in range(2):
        sh = 10 * m                                # second slot: pattern shifted by 10 columns
        f["uu"][m] = (20.0 * clat * (1.0 + 0.3 * _wave(k, nz))
                      + 5.0 * _wave(3 * (i + sh), per) + 0.0 * j)
        f["vv"][m] = 5.0 * _wave(2 * (i + sh) + 0 * j, per) * clat + 1.5 * _wave(k + 3 * j, 40)
        f["ww"][m] = (0.05 * _wave(i + sh, per) * _wave(2 * j + 0 * i, ny - 1)
                      * 4.0 * zf * (1.0 - zf))
        r = (1.2 + 0.02 * m) / den + 0.0 * (i + j)
        f["rho"][m] = r * (1.0 + 0.01 * _wave(i + 2 * j, per))
        f["drhodz"][m] = -(1.2 + 0.02 * m) * (1.0 + a) / 8000.0 / (den * den) + 0.0 * (i + j)
        f["tt"][m] = np.maximum(288.0 - 0.0065 * z + 2.0 * _wave(i + sh + j, per), 216.0)
    i2 = i[0]; j2 = j[0]; c2 = clat[0]
    f["hmix"] = np.empty(shp2); f["ustar"] = np.empty(shp2); f["wstar"] = np.empty(shp2)
    f["oli"] = np.empty(shp2); f["tropopause"] = np.empty(shp2)
    f["vdep"] = np.empty((2, nspec, ny, nx))
    for m in range(2):
        sh = 10 * m
        if hmix_const is not None:
            f["hmix"][m] = float(hmix_const)
        else:
            hm = 300.0 + 1200.0 * (0.5 + 0.5 * _wave(i2 + sh, per) * c2) + 300.0 * _wave(3 * j2 + i2, 64)
            f["hmix"][m] = np.minimum(np.maximum(hm, HMIXMIN), HMIXMAX)
        f["ustar"][m] = 0.1 + 0.4 * c2 + 0.05 * _wave(5 * (i2 + sh), per)
        olw = _wave(2 * (i2 + sh) + j2, per)
        f["oli"][m] = 0.02 * olw * (0.25 + 0.75 * c2)
        # convective velocity scale: sizeable where the surface layer is unstable (1/L < 0),
        # small but non-zero elsewhere (the CBL scheme divides by powers of w*)
        f["wstar"][m] = 0.1 + 1.9 * np.maximum(0.0, -olw) + 0.0 * c2
        f["tropopause"][m] = 9000.0 + 7000.0 * c2 + 0.0 * i2
        for ks in range(nspec):
            f["vdep"][m, ks] = 0.002 * (ks + 1) + 0.001 * _wave(i2 + sh + j2, per)
    if xcyclic_ok(nx):
        for key in ("uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli",
                    "tropopause", "vdep"):
            f[key][..., nx - 1] = f[key][..., 0]   # cyclic duplicate column (gridcheck: nx = nxfield+1)
    if polar:
        # any smooth field serves parity: the real ones come from verttransform (out of scope)
        f["uupol"] = 0.7 * f["uu"] + 0.2 * f["vv"]
        f["vvpol"] = 0.7 * f["vv"] - 0.2 * f["uu"]
    return f


def xcyclic_ok(nx):
    return nx >= 3


# --------------------------------------------------------------------------
# particles
# --------------------------------------------------------------------------
def make_particles(n, nx, ny, height, hmix, *, seed=0x5EED, lat_margin_cells=None,
                   frac_pbl=0.5, zmax=12000.0, nspec=1, itime0=0):
    """Fixed-seed particle cloud over the whole grid.

    Half the particles (frac_pbl) are placed below the local mixing height so
    that both branches of the trajectory step are exercised.
    """
    ux = _uniform01(n, seed + 1)
    uy = _uniform01(n, seed + 2)
    uz = _uniform01(n, seed + 3)
    us = _uniform01(n, seed + 4)
    eps = 361.0 / 3.0e5
    if lat_margin_cells is None:
        lat_margin_cells = 0.03 * (ny - 1)
    x = eps + ux * (float(nx - 1) - 2.0 * eps)
    y = lat_margin_cells + uy * (float(ny - 1) - 2.0 * lat_margin_cells)
    ix = np.minimum(x.astype(np.int64), nx - 2)
    jy = np.minimum(y.astype(np.int64), ny - 2)
    hloc = np.maximum.reduce([hmix[0, jy, ix], hmix[0, jy, ix + 1], hmix[0, jy + 1, ix],
                              hmix[0, jy + 1, ix + 1], hmix[1, jy, ix], hmix[1, jy, ix + 1],
                              hmix[1, jy + 1, ix], hmix[1, jy + 1, ix + 1]])
    in_pbl = us < frac_pbl
    z = np.where(in_pbl, 10.0 + uz * np.maximum(hloc - 20.0, 1.0),
                 hloc + 10.0 + uz * (zmax - hloc - 10.0))
    p = dict(npart=n, xtra1=x, ytra1=y, ztra1=z,
             itra1=np.full(n, itime0, np.int32), itramem=np.full(n, itime0, np.int32),
             npoint=np.ones(n, np.int32), nclass=np.ones(n, np.int32),
             xmass1=np.ones((nspec, n), np.float64))
    return p


def point_release(n, xlon, ylat, z, dx, dy, xlon0, ylat0, *, nspec=1, itime0=0):
    """All particles at one point (options/RELEASES default case of the reference)."""
    x = np.full(n, (xlon - xlon0) / dx)
    y = np.full(n, (ylat - ylat0) / dy)
    return dict(npart=n, xtra1=x, ytra1=y, ztra1=np.full(n, float(z)),
                itra1=np.full(n, itime0, np.int32), itramem=np.full(n, itime0, np.int32),
                npoint=np.ones(n, np.int32), nclass=np.ones(n, np.int32),
                xmass1=np.full((nspec, n), 1.0 / n))


# --------------------------------------------------------------------------
# scenarios
# --------------------------------------------------------------------------
def base_scenario(nx=361, ny=181, nz=138, *, global_grid=True, polar=False, nspec=1,
                  ctl=5.0, ifine=4, cblflag=0, lsynctime=900, uniform=None, hmix_const=None,
                  turb_off=False, nsteps=2, ldirect=1):
    """Grid + switches + fields; particles are added by the caller."""
    height = make_height(nz, top=80000.0 if nz >= 60 else 30000.0,
                         lin=0.05 if nz >= 60 else 0.15)
    dx = 360.0 / (nx - 1) if global_grid else 1.0
    dy = 180.0 / (ny - 1) if global_grid else 1.0
    xlon0 = -180.0 if global_grid else -20.0
    ylat0 = -90.0 if global_grid else 20.0
    sw = derive_switches(ctl, ifine, cblflag, lsynctime)
    sc = dict(
        grid=np.array([nx, ny, nz], np.int32),
        geom=np.array([dx, dy, xlon0, ylat0], np.float64),
        globalflags=np.array([int(global_grid), int(global_grid and polar),
                              int(global_grid and polar)], np.int32),
        height=height, nmixz=nmixz_from_height(height),
        # backward runs: lsynctime and the wind window run towards negative times (readcommand.f90:631,
        # getfields.f90 orders wftime by ldirect); mintime stays positive (readcommand.f90:381-384 come first)
        memtime=np.array([0, 10800 * ldirect], np.int32), memind=np.array([1, 2], np.int32),
        ldirect=ldirect, lsynctime=sw["lsynctime"] * ldirect, method=sw["method"], mintime=sw["mintime"],
        ctl=sw["ctl"], ifine=sw["ifine"], turbswitch=sw["turbswitch"], cblflag=sw["cblflag"],
        mdomainfill=0, lsettling=0, nspec=nspec,
        drydep=0, drydepspec=np.zeros(nspec, np.int32),
        density=np.zeros(nspec), dquer=np.zeros(nspec), vsetaver=np.zeros(nspec),
        cunningham=np.ones(nspec), decay=np.zeros(nspec),
        turbpar=np.array([0.0, 0.0, 0.0]) if turb_off else np.array([50.0, 0.1, 0.16]),
        lage=np.array([999999999], np.int32),
        nsteps=nsteps, itime0=0,
    )
    sc.update(make_fields(nx, ny, nz, height, uniform=uniform, polar=polar, nspec=nspec,
                          hmix_const=hmix_const))
    return sc


def config1(n=10000, nsteps=2):
    """BASELINE config 1: 10k particles, point release, uniform wind, no turbulence.

    Uniform values of the reference's own validation set (mpi_mod.f90:2940-2973: u=10, v=0,
    w=0, rho=1.3); 'no turbulence' is obtained the reference's run-time way (SURVEY appendix
    A): particles above the mixing height and d_trop = d_strat = turbmesoscale = 0.
    """
    sc = base_scenario(uniform=dict(u=10.0, v=0.0, w=0.0, rho=1.3, hmix=HMIXMIN, ustar=1.0,
                                    wstar=1.0, oli=0.01, tropopause=10000.0),
                       ctl=-5.0, ifine=4, turb_off=True, nsteps=nsteps)
    g = sc["geom"]
    sc.update(point_release(n, 0.0, 20.0, 150.0, g[0], g[1], g[2], g[3]))
    return sc


def config2(n=10_000_000, nsteps=2, seed=0x5EED, nx=361, ny=181, nz=138):
    """BASELINE config 2: advance + interpol_wind only (all particles above the PBL)."""
    sc = base_scenario(nx, ny, nz, ctl=-5.0, ifine=4, turb_off=True, hmix_const=HMIXMIN,
                       nsteps=nsteps)
    sc.update(make_particles(n, nx, ny, sc["height"], sc["hmix"], seed=seed, frac_pbl=0.0))
    return sc


def config3(n=100_000_000, nsteps=2, seed=0x5EED, nx=361, ny=181, nz=138, cblflag=1,
            ctl=5.0, ifine=4):
    """BASELINE config 3: full Hanna turbulence + CBL, PBL sub-stepping."""
    sc = base_scenario(nx, ny, nz, ctl=ctl, ifine=ifine, cblflag=cblflag, nsteps=nsteps)
    sc.update(make_particles(n, nx, ny, sc["height"], sc["hmix"], seed=seed, frac_pbl=0.5))
    return sc


def small(n=2000, nx=40, ny=24, nz=30, **kw):
    """A small grid + cloud for fast parity tests (same generators, reduced sizes)."""
    cbl = kw.pop("cblflag", 0)
    ctl = kw.pop("ctl", 5.0)
    ifine = kw.pop("ifine", 4)
    nsteps = kw.pop("nsteps", 3)
    seed = kw.pop("seed", 1234)
    frac_pbl = kw.pop("frac_pbl", 0.5)
    zmax = kw.pop("zmax", 12000.0)
    lat_margin = kw.pop("lat_margin_cells", None)
    sc = base_scenario(nx, ny, nz, ctl=ctl, ifine=ifine, cblflag=cbl, nsteps=nsteps, **kw)
    sc.update(make_particles(n, nx, ny, sc["height"], sc["hmix"], seed=seed, frac_pbl=frac_pbl,
                             zmax=zmax, nspec=int(sc["nspec"]), lat_margin_cells=lat_margin))
    return sc


def add_outgrid(sc, nxg=36, nyg=18, nzg=5, *, outlon0=None, outlat0=None, dxout=None, dyout=None,
                ind_samp=-1, old_fraction=0.5, age=20000):
    """Output grid of the concentration sampling (OUTGRID namelist shape, readoutgrid.f90) plus
    a share of particles released `age` seconds ago, so that both the direct-cell and the
    4-cell-kernel branch of conccalc (conccalc.f90:171) are exercised."""
    nx, ny, _ = (int(v) for v in sc["grid"])
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    if outlon0 is None:
        outlon0 = xlon0 + 0.05 * (nx - 1) * dx
    if outlat0 is None:
        outlat0 = ylat0 + 0.10 * (ny - 1) * dy
    if dxout is None:
        dxout = 0.9 * (nx - 1) * dx / nxg
    if dyout is None:
        dyout = 0.8 * (ny - 1) * dy / nyg
    sc["outgrid"] = np.array([nxg, nyg, nzg], np.int32)
    sc["outgeom"] = np.array([dxout, dyout, outlon0, outlat0], np.float64)
    sc["outheight"] = np.array([100.0, 500.0, 1500.0, 5000.0, 20000.0][:nzg] if nzg <= 5
                               else 100.0 * (np.arange(nzg) + 1.0) ** 2)
    sc["concflags"] = np.array([ind_samp, 0], np.int32)
    sc["outtimes"] = np.array([3600, 3600], np.int32)
    n = int(sc["npart"])
    old = _uniform01(n, 0xA6E) < old_fraction
    itramem = np.asarray(sc["itramem"]).copy()
    itramem[old] = int(sc["itime0"]) - int(age)
    sc["itramem"] = itramem.astype(np.int32)
    return sc


def add_release_points(sc, xmass, npart_rel, *, ioutputforeachrelease=1, lage=None, max_age=None,
                       nclassunc=1, tiny_every=0, tiny_factor=5.0e-5, near_every=0, near_factor=1.03e-4):
    """Several release points (RELEASES with more than one &RELEASE block): point_mod xmass(numpoint,nspec)
    (given as [nspec][numpoint]) and npart(numpoint); every particle gets a release point npoint(j), the mass
    xmass(kp,ks)/npart(kp) of its point (readreleases.f90 / releaseparticles.f90:148-155), an uncertainty class
    nclass(j) in 1..nclassunc and -- with max_age -- a release time up to max_age seconds before the start, so
    that particles fall into several age classes and some exceed lage(nageclass) (timemanager.f90:701-707).
    tiny_every / near_every: every k-th particle carries tiny_factor / near_factor of its nominal mass, i.e. lies
    below / just above minmass = 1e-4 (par_mod.f90:213) of it: terminated at once / after some decay
    (timemanager.f90:681-686)."""
    nspec = int(sc["nspec"])
    xm = np.asarray(xmass, dtype=np.float64).reshape(nspec, -1)
    numpoint = xm.shape[1]
    npt = np.asarray(npart_rel, dtype=np.int32).ravel()
    assert npt.size == numpoint
    n = int(sc["npart"])
    h = _splitmix64(n, 0xBEEF)
    kp = (h % np.uint64(numpoint)).astype(np.int64)                  # 0-based release point
    sc["numpoint"] = numpoint
    sc["xmass"] = xm
    sc["npart_rel"] = npt
    sc["npoint"] = (kp + 1).astype(np.int32)
    m = xm[:, kp] / npt[kp].astype(np.float64)[None, :]
    idx = np.arange(n)
    if tiny_every:
        m[:, idx % tiny_every == 1] *= tiny_factor
    if near_every:
        m[:, idx % near_every == 2] *= near_factor
    sc["xmass1"] = m
    sc["nclassunc"] = int(nclassunc)
    sc["nclass"] = (1 + ((h >> np.uint64(20)) % np.uint64(nclassunc)).astype(np.int64)).astype(np.int32)
    if lage is not None:
        sc["lage"] = np.asarray(lage, np.int32)
    if max_age:
        age = ((h >> np.uint64(32)) % np.uint64(int(max_age))).astype(np.int64)
        sc["itramem"] = (int(sc["itime0"]) - age * int(sc["ldirect"])).astype(np.int32)
    if "concflags" in sc:
        sc["concflags"] = np.array([int(sc["concflags"][0]), int(ioutputforeachrelease)], np.int32)
    return sc


def add_outgrid_nest(sc, nxn=30, nyn=20):
    """Nested output grid (OUTGRID_NEST, readoutgrid_nest.f90): finer cells over the middle of the
    mother output grid, so that particles fall inside, on its border and outside of it."""
    nxg, nyg, _ = (int(v) for v in sc["outgrid"])
    dxout, dyout, outlon0, outlat0 = (float(v) for v in sc["outgeom"])
    sc["outgridn"] = np.array([nxn, nyn], np.int32)
    sc["outgeomn"] = np.array([0.4 * nxg * dxout / nxn, 0.5 * nyg * dyout / nyn,
                               outlon0 + 0.3 * nxg * dxout, outlat0 + 0.25 * nyg * dyout], np.float64)
    return sc


def add_receptors(sc, m=4):
    """Receptor points (RECEPTORS, readreceptors.f90:88-92): positions in grid coordinates and the
    area of a dx*dy cell there; placed on particles so that the parabolic kernel finds some."""
    x = np.asarray(sc["xtra1"], dtype=np.float64)
    y = np.asarray(sc["ytra1"], dtype=np.float64)
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    idx = (np.arange(m, dtype=np.int64) * 7919 + 11) % x.size
    xr = np.float32(x[idx]).astype(np.float64)
    yr = np.float32(y[idx]).astype(np.float64)
    r_earth, pi180 = 6.371e6, 3.14159265 / 180.0
    ylat = ylat0 + yr * dy
    area = (r_earth * np.cos(ylat * pi180) * dx * pi180) * (r_earth * dy * pi180)
    sc["receptors"] = np.concatenate([xr, yr, np.float32(area).astype(np.float64)])
    return sc


def _wet_fields(nx, ny, nz, z, phase):
    """lsprec, convprec, tcc [2][ny][nx]; clouds [2][nz][ny][nx]; cloudsh [2][ny][nx] (exact arithmetic)."""
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, :]
    j = np.arange(ny, dtype=np.int64)[:, None]
    lsprec = np.empty((2, ny, nx)); convprec = np.empty((2, ny, nx)); tcc = np.empty((2, ny, nx))
    clouds = np.zeros((2, nz, ny, nx), np.int32)
    cloudsh = np.zeros((2, ny, nx), np.int32)
    for m in range(2):
        sh = 7 * m + phase
        lsprec[m] = 12.0 * np.maximum(0.0, _wave(2 * (i + sh) + j, per)) ** 2
        convprec[m] = 6.0 * np.maximum(0.0, _wave(3 * (i + sh) + 2 * j, per))
        tcc[m] = 0.15 + 0.8 * np.abs(_wave(i + sh + 3 * j, per))
        raining = (lsprec[m] + convprec[m]) > 0.01
        for k in range(nz):
            cls = 6 if z[k] < 1200.0 else (3 if z[k] < 5000.0 else 0)
            clouds[m, k] = np.where(raining, cls, 0)
        cloudsh[m] = np.where(raining, 3800, 0)
    return lsprec, convprec, tcc, clouds, cloudsh


def add_wet_nest(sc):
    """The nest's own precipitation, cloud and temperature fields (lsprecn, convprecn, tccn, cloudsn,
    cloudshn, ttn; get_wetscav.f90:126-128,150-151,197-199); after add_nest and add_wet."""
    nxn, nyn = (int(v) for v in sc["nest"])
    nz = int(sc["grid"][2])
    lsp, cvp, tcc, cl, clh = _wet_fields(nxn, nyn, nz, np.asarray(sc["height"]), 3)
    f = make_fields(nxn, nyn, nz, sc["height"], nspec=int(sc["nspec"]))
    sc.update(lsprecn=lsp, convprecn=cvp, tccn=tcc, cloudsn=cl, cloudshn=clh, ttn=f["tt"] - 4.0)
    return sc


def add_wet(sc, *, gas=False):
    """Precipitation / cloud fields and wet-scavenging species parameters (readspecies.f90 names).

    clouds (int8 per level, verttransform's cloud classification): >= 4 below a precipitating
    cloud, 2-3 inside it, 0-1 none (get_wetscav.f90:150,206,251).  gas=False: an aerosol
    (dquer > 0, crain/csnow below cloud, ccn/in inside); gas=True: a soluble gas (weta/wetb,
    henry)."""
    nx, ny, nz = (int(v) for v in sc["grid"])
    lsprec, convprec, tcc, clouds, cloudsh = _wet_fields(nx, ny, nz, np.asarray(sc["height"]), 0)
    sc.update(lsprec=lsprec, convprec=convprec, tcc=tcc, clouds=clouds, cloudsh=cloudsh, wetdep=1,
              wetdepspec=np.array([1], np.int32))
    if gas:
        sc.update(weta_gas=np.array([2.0e-5]), wetb_gas=np.array([0.62]), crain_aero=np.array([0.0]),
                  csnow_aero=np.array([0.0]), ccn_aero=np.array([0.0]), in_aero=np.array([0.0]),
                  henry=np.array([1.0e5]))
    else:
        sc.update(weta_gas=np.array([0.0]), wetb_gas=np.array([0.0]), crain_aero=np.array([1.0]),
                  csnow_aero=np.array([1.0]), ccn_aero=np.array([0.9]), in_aero=np.array([0.1]),
                  henry=np.array([0.0]))
        if float(np.asarray(sc["dquer"])[0]) <= 0.0:
            sc["dquer"] = np.array([8.0])
    return sc


def add_nest(sc, ix0=None, jy0=None, ix1=None, jy1=None, factor=2):
    """One nested grid of `factor` times the mother resolution over mother cells [ix0,ix1]x[jy0,jy1]
    (com_mod.f90:464-541 arrays uun, vvn, ... ; geometry as gridcheck_nests.f90 derives it)."""
    nx, ny, nz = (int(v) for v in sc["grid"])
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    ix0 = nx // 4 if ix0 is None else ix0
    ix1 = (2 * nx) // 3 if ix1 is None else ix1
    jy0 = ny // 4 if jy0 is None else jy0
    jy1 = (3 * ny) // 4 if jy1 is None else jy1
    nxn = factor * (ix1 - ix0) + 1
    nyn = factor * (jy1 - jy0) + 1
    f = make_fields(nxn, nyn, nz, sc["height"], nspec=int(sc["nspec"]))
    sc["nest"] = np.array([nxn, nyn], np.int32)
    sc["nestgeom"] = np.array([dx / factor, dy / factor, xlon0 + ix0 * dx, ylat0 + jy0 * dy], np.float64)
    for k, kn in (("uu", "uun"), ("vv", "vvn"), ("ww", "wwn"), ("rho", "rhon"), ("drhodz", "drhodzn"),
                  ("hmix", "hmixn"), ("ustar", "ustarn"), ("wstar", "wstarn"), ("oli", "olin"),
                  ("tropopause", "tropopausen"), ("vdep", "vdepn")):
        sc[kn] = f[k] * (1.1 if k in ("uu", "vv") else 1.0)   # not the mother's values: a wrong grid choice shows
    sc["par_nxmax"] = 721        # the reference variant with nests is built from par_mod_meteoswiss.f90
    return sc


# --------------------------------------------------------------------------
# model-level input of verttransform_ecmwf
# --------------------------------------------------------------------------
def model_levels(nx=361, ny=181, nz=138, *, global_grid=True, polar=False, phase=0):
    """ECMWF-shaped hybrid-level input as readwind_ecmwf leaves it: level 1 = surface,
    pressure of level k = akz[k] + bkz[k]*ps, nuvz = nwz = nz (gridcheck_ecmwf.f90 adds the
    surface level and sets nz = nuvz).  Arrays are compact [nz][ny][nx]; `phase` shifts the
    pattern (a second time slot).  Mountains (low ps) give columns whose top lies below the
    reference column's, which exercises the copy-the-top-level branch of the transform."""
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, None, :] + int(phase)
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    s = np.arange(ny, dtype=np.float64)[None, :, None] / float(ny - 1)
    clat = 4.0 * s * (1.0 - s)
    # hybrid coefficients: eta from 1 (surface) to exp(-7) (about 90 Pa), layers thinnest at the ground
    eta = np.exp(-7.0 * (np.arange(nz, dtype=np.float64) / float(nz - 1)) ** 1.6)
    bk = eta ** 1.5
    bk[0] = 1.0
    ak = 101325.0 * (eta - bk)
    ak[0] = 0.0
    # surface pressure: a few 'mountain ranges' down to about 620 hPa, most columns above 1000 hPa
    mount = np.maximum(0.0, _wave(2 * i[0] + 3 * j[0], per)) * np.maximum(0.0, _wave(3 * j[0] + 7, 2 * (ny - 1)))
    ps = 101500.0 + 800.0 * _wave(i[0] + 2 * j[0], per) - 39000.0 * mount * mount
    lnp = np.log((ak[:, None, None] + bk[:, None, None] * ps[None]) / 101325.0)       # <= ~0
    zapprox = -7400.0 * lnp
    tth = np.maximum(288.0 - 0.0065 * zapprox, 216.0) + 3.0 * _wave(i + j + 2 * k, per) + 10.0 * (clat - 0.5)
    qvh = 0.012 * np.exp(-zapprox / 2500.0) * (0.6 + 0.4 * _wave(2 * i + j, per))
    uuh = 25.0 * clat * (1.0 + 0.3 * _wave(k, nz)) + 6.0 * _wave(3 * i, per) + 0.0 * j
    vvh = 6.0 * _wave(2 * i + 0 * j, per) * clat + 2.0 * _wave(k + 3 * j, 40)
    wwh = 0.4 * _wave(i, per) * _wave(2 * j + 0 * i, ny - 1) * np.exp(lnp)            # eta-dot * dp/deta, Pa/s
    pvh = 1.0e-6 * (1.0 + 0.5 * _wave(i + k, per)) * np.exp(zapprox / 12000.0) * (2.0 * s - 1.0)
    tt2 = tth[0] + 0.5 * _wave(3 * i[0] + j[0], per)
    td2 = tt2 - 3.0 - 2.0 * (1.0 + _wave(i[0] + 5 * j[0], per))
    out = dict(akz=ak, bkz=bk, aknew=ak.copy(), bknew=bk.copy(), ps=ps, tt2=tt2, td2=td2,
               tth=tth, qvh=qvh, uuh=uuh, vvh=vvh, pvh=pvh, wwh=wwh)
    if xcyclic_ok(nx) and global_grid:
        for key in ("ps", "tt2", "td2", "tth", "qvh", "uuh", "vvh", "pvh", "wwh"):
            out[key][..., nx - 1] = out[key][..., 0]
    dx = 360.0 / (nx - 1) if global_grid else 1.0
    dy = 180.0 / (ny - 1) if global_grid else 1.0
    out["grid"] = np.array([nx, ny, nz], np.int32)
    out["geom"] = np.array([dx, dy, -180.0 if global_grid else -20.0, -90.0 if global_grid else 20.0], np.float64)
    out["globalflags"] = np.array([int(global_grid), int(global_grid and polar), int(global_grid and polar)], np.int32)
    return out


# --------------------------------------------------------------------------
# pressure-level input of verttransform_gfs (NCEP GFS)
# --------------------------------------------------------------------------
# the pressure levels of the GFS GRIB files [hPa], bottom up (the 26 classic ones are 1000 ... 10 without 40, 15, 7 ...)
GFS_PLEV_HPA = (1000., 975., 950., 925., 900., 850., 800., 750., 700., 650., 600., 550., 500., 450., 400., 350., 300., 250., 200.,
                150., 100., 70., 50., 40., 30., 20., 15., 10., 7., 5., 3., 2., 1., 0.7, 0.4, 0.2, 0.1, 0.07, 0.04, 0.02, 0.01)


def gfs_levels(nx=361, ny=181, nz=34, *, global_grid=True, polar=False, phase=0, terrain=0.0):
    """NCEP-GFS-shaped pressure-level input as readwind_gfs / gridcheck_gfs leave it: akz = the pressures of the lowest nz
    GFS levels (descending), bkz = 0, aknew = akz, bknew = 0, nuvz = nwz = nz (gridcheck_gfs.f90:439-491).  Arrays are
    compact [nz][ny][nx]; levels below the ground carry (extrapolated) values, as in the GRIB files; `phase` shifts the
    pattern (another wind field).
    terrain: depth [Pa] of the deepest surface-pressure depression ('mountain').  terrain = 0: every ps lies between akz[1]
    and akz[0] = 1000 hPa except one column above 1000 hPa (the column the z levels are built from); terrain > 0: ps runs
    from about 1030 hPa down to about 1030 hPa - terrain, so the first level above ground (llev of verttransform_gfs.f90:
    149-154) differs from column to column and low-ps columns end below the top of the reference column.
    Half of the columns have a lapse rate near zero, so that both outcomes of |tv - tvold| > 0.2 (:174) occur."""
    if not 4 <= nz <= len(GFS_PLEV_HPA):
        raise ValueError("gfs_levels: 4 <= nz <= %d" % len(GFS_PLEV_HPA))
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, None, :] + int(phase)
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    s = np.arange(ny, dtype=np.float64)[None, :, None] / float(ny - 1)
    clat = 4.0 * s * (1.0 - s)
    ak = 100.0 * np.array(GFS_PLEV_HPA[:nz], np.float64)
    # 'mountain ranges' in rows 4 ... 3 + (ny-1)/2 only: the rows next to the pole rows stay flat
    mount = np.maximum(0.0, _wave(2 * i[0] + 3 * j[0], per)) * np.maximum(0.0, _wave(j[0] - 3, ny - 1))
    if terrain > 0.0:
        ps = 102200.0 + 800.0 * _wave(i[0] + 2 * j[0], per) - float(terrain) * mount * mount
    else:
        ps = 98900.0 + 600.0 * _wave(i[0] + 2 * j[0], per) + 0.0 * j[0]
        ps[1, 1] = 100600.0
    zapprox = -7400.0 * np.log(ak / 101325.0)[:, None, None]
    lam = np.maximum(0.0, _wave(i + 3 * j, per))                                   # lapse-rate factor: 0 over half the columns
    tth = 288.0 - 0.0065 * zapprox * lam + 3.0 * _wave(i + j, per) + 10.0 * (clat - 0.5) + 0.0 * k
    qvh = 0.004 * np.exp(-zapprox / 2500.0) * (0.6 + 0.4 * _wave(2 * i + j, per))
    uuh = 25.0 * clat * (1.0 + 0.3 * _wave(k, nz)) + 6.0 * _wave(3 * i, per) + 0.0 * j
    vvh = 6.0 * _wave(2 * i + 0 * j, per) * clat + 2.0 * _wave(k + 3 * j, 10) + 0.0 * i   # both signs on the pole rows
    wwh = 0.4 * _wave(i, per) * _wave(2 * j + 0 * i, ny - 1) * (ak / 101325.0)[:, None, None]
    pvh = 1.0e-6 * (1.0 + 0.5 * _wave(i + k, per)) * np.exp(zapprox / 12000.0) * (2.0 * s - 1.0)
    tt2 = tth[0] + 0.5 * _wave(3 * i[0] + j[0], per)
    td2 = tt2 - 3.0 - 2.0 * (1.0 + _wave(i[0] + 5 * j[0], per))
    out = dict(akz=ak, bkz=np.zeros(nz), aknew=ak.copy(), bknew=np.zeros(nz), ps=ps, tt2=tt2, td2=td2,
               tth=tth, qvh=qvh, uuh=uuh, vvh=vvh, pvh=pvh, wwh=wwh)
    if xcyclic_ok(nx) and global_grid:
        for key in ("ps", "tt2", "td2", "tth", "qvh", "uuh", "vvh", "pvh", "wwh"):
            out[key][..., nx - 1] = out[key][..., 0]
    dx = 360.0 / (nx - 1) if global_grid else 1.0
    dy = 180.0 / (ny - 1) if global_grid else 1.0
    out["grid"] = np.array([nx, ny, nz], np.int32)
    out["geom"] = np.array([dx, dy, -180.0 if global_grid else -20.0, -90.0 if global_grid else 20.0], np.float64)
    out["globalflags"] = np.array([int(global_grid), int(global_grid and polar), int(global_grid and polar)], np.int32)
    return out


# --------------------------------------------------------------------------
# particle dump (partoutput.f90): the extra fields it interpolates
# --------------------------------------------------------------------------
def add_partoutput_fields(sc, itime=None, dead_every=7):
    """oro, pv, qv for a scenario that already has height, rho, tt, hmix, tropopause and particles; every
    `dead_every`-th particle is made not due (terminated) so that the dump has to skip it."""
    nx, ny, nz = (int(v) for v in sc["grid"])
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    z = np.asarray(sc["height"], dtype=np.float64)[:, None, None]
    sc["oro"] = 400.0 * (1.0 + _wave(2 * i[0] + 3 * j[0], per)) + 0.0 * j[0]
    pv = np.empty((2, nz, ny, nx)); qv = np.empty((2, nz, ny, nx))
    for m in range(2):
        sh = 10 * m
        pv[m] = 1.0e-6 * (1.0 + 0.5 * _wave(i + sh + k, per)) * (1.0 + z / 6000.0) * (2.0 * j / float(ny - 1) - 1.0)
        qv[m] = 0.012 / (1.0 + z / 2500.0) ** 2 * (0.6 + 0.4 * _wave(2 * (i + sh) + j, per)) + 0.0 * k
    if xcyclic_ok(nx):
        pv[..., nx - 1] = pv[..., 0]; qv[..., nx - 1] = qv[..., 0]; sc["oro"][..., nx - 1] = sc["oro"][..., 0]
    sc["pv"] = pv; sc["qv"] = qv
    it = int(sc.get("itime0", 0)) if itime is None else int(itime)
    sc["itime"] = it
    itra1 = np.full(int(sc["npart"]), it, np.int32)
    if dead_every:
        itra1[::dead_every] = -999999999
    sc["itra1"] = itra1
    sc["npoint"] = (1 + np.arange(int(sc["npart"])) % 3).astype(np.int32)
    return sc


def nest_model_levels(m, ix0=10, jy0=6, ix1=25, jy1=16, factor=2, phase=3):
    """Model-level input on one nested grid covering mother cells [ix0,ix1] x [jy0,jy1] at `factor` times the
    resolution (verttransform_nests.f90); same hybrid coefficients as the mother, its own smooth patterns."""
    nx, ny, nz = (int(v) for v in m["grid"])
    dx, dy, xlon0, ylat0 = (float(v) for v in m["geom"])
    nxn, nyn = (ix1 - ix0) * factor + 1, (jy1 - jy0) * factor + 1
    n = model_levels(nx=nxn, ny=nyn, nz=nz, global_grid=False, polar=False, phase=phase)
    for k in ("akz", "bkz", "aknew", "bknew"):
        n[k] = m[k].copy()
    n["geom"] = np.array([dx / factor, dy / factor, xlon0 + ix0 * dx, ylat0 + jy0 * dy], np.float64)
    n["globalflags"] = np.array([0, 0, 0], np.int32)
    return n


# --------------------------------------------------------------------------
# concoutput: output grids with the run structure the sparse writer compresses
# --------------------------------------------------------------------------
def concoutput_case(nxg=24, nyg=16, nzg=4, nspec=2, wet=True, dry=True, itime=3600, seed=5, classes=1):
    """gridunc / wetgridunc / drygridunc with empty stretches, single cells and long runs (float32 values, as the
    sampling kernels leave them), plus area/volume as outgrid_init.f90:59-95 computes them.  classes > 1: the grids carry
    a leading uncertainty-class dimension [classes][nspec]... (nclassunc of par_mod; concoutput writes the class mean times
    nclassunc, concoutput.f90:296-345 with mean_mod)."""
    if classes > 1:
        parts = [concoutput_case(nxg, nyg, nzg, nspec, wet, dry, itime, seed + 17 * c) for c in range(classes)]
        co = dict(parts[0])
        co["classes"] = np.array([classes], np.int32)
        for k in ("gridunc", "wetgridunc", "drygridunc"):
            if k in co:
                co[k] = np.stack([p[k] for p in parts])
        return co
    u = _uniform01(nspec * nzg * nyg * nxg, seed).reshape(nspec, nzg, nyg, nxg)
    blob = _wave(np.arange(nxg)[None, None, None, :] * 3 + np.arange(nyg)[None, None, :, None] * 5, 4 * nxg)
    g = np.where((u > 0.55) & (blob > -0.2), (u * 1.0e-3).astype(np.float32), np.float32(0.0)).astype(np.float64)
    g[:, :, 0, :] = 0.0                      # a whole empty row
    g[:, 1, 3, :] = 2.0e-4                   # a whole full row
    w2 = np.where(u[:, 0] > 0.7, (u[:, 0] * 1.0e-5).astype(np.float32), np.float32(0.0)).astype(np.float64)
    d2 = np.where(u[:, 1] > 0.4, (u[:, 1] * 1.0e-6).astype(np.float32), np.float32(0.0)).astype(np.float64)
    outheight = np.array([100.0, 500.0, 1000.0, 5000.0, 10000.0, 15000.0, 20000.0, 25000.0, 30000.0, 40000.0, 50000.0, 60000.0][:nzg])
    dxout, dyout, outlon0, outlat0 = 1.0, 1.0, -10.0, 30.0
    f32 = np.float32
    pi, r_earth = f32(3.14159265), f32(6.371e6)
    pi180 = pi / f32(180.0)
    area = np.zeros((nyg, nxg)); volume = np.zeros((nzg, nyg, nxg))
    for jy in range(nyg):                    # outgrid_init.f90:59-95 in the reference's own real kind (f32)
        ylat = f32(outlat0) + (f32(jy) + f32(0.5)) * f32(dyout)
        ylatp = ylat + f32(0.5) * f32(dyout); ylatm = ylat - f32(0.5) * f32(dyout)
        if ylatm < 0 and ylatp > 0:
            hzone = f32(dyout) * r_earth * pi180
        else:
            cp = f32(np.cos(ylatp * pi180)); cm = f32(np.cos(ylatm * pi180))
            a_, b_ = (cp, cm) if cp < cm else (cm, cp)
            hzone = (f32(np.sqrt(f32(1) - a_ * a_)) - f32(np.sqrt(f32(1) - b_ * b_))) * r_earth
        ga = f32(2.0) * pi * r_earth * hzone * f32(dxout) / f32(360.0)
        area[jy, :] = ga
        volume[0, jy, :] = ga * f32(outheight[0])
        for kz in range(1, nzg):
            volume[kz, jy, :] = ga * (f32(outheight[kz]) - f32(outheight[kz - 1]))
    co = dict(outgrid=np.array([nxg, nyg, nzg, nspec, int(wet), int(dry), itime], np.int32),
              outgeom=np.array([dxout, dyout, outlon0, outlat0, 4.0]), outheight=outheight, area=area, volume=volume, gridunc=g)
    if wet:
        co["wetgridunc"] = w2
    if dry:
        co["drygridunc"] = d2
    return co


def add_pptv(co, nx=40, ny=24, nz=12):
    """Mixing-ratio output (iout = 3) for a concoutput_case(): a met grid that covers the output grid, z levels, the air
    density of slot memind(2) and molar weights (concoutput.f90:176-205,482-590)."""
    nxg, nyg = int(co["outgrid"][0]), int(co["outgrid"][1])
    dxout, dyout, outlon0, outlat0 = (float(v) for v in co["outgeom"][:4])
    co["iout"] = 3
    co["met"] = np.array([nx, ny, nz], np.int32)
    co["metgeom"] = np.array([(nxg * dxout + 2.0) / (nx - 1), (nyg * dyout + 2.0) / (ny - 1), outlon0 - 1.0, outlat0 - 1.0])
    co["height"] = make_height(nz, top=30000.0, lin=0.15)
    i = np.arange(nx, dtype=np.int64)[None, None, :]; j = np.arange(ny, dtype=np.int64)[None, :, None]
    z = np.asarray(co["height"])[:, None, None]
    co["rho2"] = (1.2 / (1.0 + z / 8000.0 + 0.5 * (z / 8000.0) ** 2) * (1.0 + 0.02 * _wave(i + 2 * j, nx - 1))).astype(np.float32).astype(np.float64)
    co["weightmolar"] = np.array([350.0, 28.0, 64.0, 100.0, 46.0][: int(co["outgrid"][3])])
    return co


# --------------------------------------------------------------------------
# releaseparticles + particle splitting
# --------------------------------------------------------------------------
def release_case(nx=48, ny=32, nz=24, *, nspec=2, ind_rel=1, mquasilag=0, maxpart=100000, itsplit=1800, existing=400,
                 times=(0, 900, 1800, 2700, 3600), global_grid=True, ibdate=20200615, ibtime=120000, nest=False):
    """RELEASES with five release points of every kind the routine distinguishes: a point source released at one
    instant (kindz 1), a box released over an interval (area source, metres above ground), a box in metres above sea
    level (kindz 2: topography subtracted), a box given in pressure (kindz 3: converted with rho and tt of time slot
    2), and a box across the date line of a global grid (the xglobal wrap).  Particles of a run in progress occupy
    the first storage spaces, some of them terminated (vacant), some due for splitting.  Local-time emission factors
    (point_hour, area_dow ...) differ per species.  nest=True: a nested wind field of twice the resolution over mother cells
    [16,32] x [6,22] with its own orography, density and temperature: the second box straddles its western edge, the box above
    sea level lies inside it, the pressure box straddles its eastern edge (releaseparticles.f90:196-226)."""
    height = make_height(nz, top=30000.0, lin=0.15)
    dx = 360.0 / (nx - 1) if global_grid else 1.0
    dy = 180.0 / (ny - 1) if global_grid else 1.0
    xlon0, ylat0 = (-180.0, -90.0) if global_grid else (-20.0, 20.0)
    f = make_fields(nx, ny, nz, height, nspec=nspec)
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, :]
    j = np.arange(ny, dtype=np.int64)[:, None]
    oro = 300.0 * (1.0 + _wave(2 * i + 3 * j, per)) + 0.0 * j
    oro[:, nx - 1] = oro[:, 0]
    rs = dict(grid=np.array([nx, ny, nz], np.int32), geom=np.array([dx, dy, xlon0, ylat0]), xglobal=int(global_grid),
              height=height, nspec=nspec, bdate=np.array([ibdate, ibtime], np.int32),
              switches=np.array([1, 900, 1, itsplit, ind_rel, mquasilag, maxpart, 1], np.int32),
              times=np.asarray(times, np.int32), oro=oro, rho2=f["rho"][1], tt2=f["tt"][1])
    # release points in grid coordinates (readreleases.f90 converts lon/lat with (x-xlon0)/dx)
    xm = nx - 1.0 if global_grid else nx - 4.0      # the last box crosses the date line of a global grid only
    rs.update(numpoint=5,
              ireleasestart=np.array([0, 0, 900, 0, 900], np.int32), ireleaseend=np.array([0, 3600, 2700, 3600, 900], np.int32),
              npart_rel=np.array([300, 1000, 800, 600, 500], np.int32), kindz=np.array([1, 1, 2, 3, 1], np.int32),
              xpoint1=np.array([10.25, 14.0, 20.5, 30.0, xm - 1.5]), xpoint2=np.array([10.25, 17.5, 24.0, 33.0, xm + 1.5]),
              ypoint1=np.array([12.5, 8.0, 18.0, 10.0, 15.0]), ypoint2=np.array([12.5, 11.0, 21.5, 13.0, 17.0]),
              zpoint1=np.array([50.0, 0.0, 900.0, 850.0, 100.0]), zpoint2=np.array([50.0, 800.0, 2500.0, 500.0, 3000.0]),
              xmass=np.array([[1.0, 5.0, 2.0, 1.5, 0.8], [0.5, 0.0, 4.0, 1.0, 0.3]][:nspec]))
    hour = 1.0 + 0.5 * _wave(np.arange(24)[:, None] * 2 + np.arange(nspec)[None, :] * 5, 24)
    dow = 1.0 + 0.25 * _wave(np.arange(7)[:, None] * 3 + np.arange(nspec)[None, :], 7)
    rs.update(point_hour=hour, area_hour=hour[::-1].copy(), point_dow=dow, area_dow=dow[::-1].copy())
    if nest:
        ix0, ix1, jy0, jy1, fac = 16, 32, 6, 22, 2
        nxn, nyn = fac * (ix1 - ix0) + 1, fac * (jy1 - jy0) + 1
        fn = make_fields(nxn, nyn, nz, height, nspec=nspec)
        gi = np.arange(nxn, dtype=np.int64)[None, :]
        gj = np.arange(nyn, dtype=np.int64)[:, None]
        rs.update(nest=np.array([nxn, nyn], np.int32), nestcorners=np.array([ix0, jy0, ix1, jy1, fac, fac], np.float64), par_nxmax=721,
                  oron=420.0 * (1.0 + _wave(3 * gi + gj, 2 * per)) + 0.0 * gj, rhon2=fn["rho"][1] * 1.03, ttn2=fn["tt"][1] - 2.5)
    if existing:
        n = int(existing)
        u = _uniform01(n, 77)
        itra1 = np.zeros(n, np.int32)                      # all synchronised at the first release time ...
        itra1[::5] = -999999999                            # ... except the terminated ones: vacant storage spaces
        itramem = -(900 * (1 + (np.arange(n) % 4))).astype(np.int32)
        rs.update(npart=n, xtra1=2.0 + u * (nx - 5.0), ytra1=2.0 + _uniform01(n, 78) * (ny - 5.0), ztra1=10.0 + 3000.0 * _uniform01(n, 79),
                  itra1=itra1, itramem=itramem, itrasplit=(itramem + itsplit).astype(np.int32),
                  npoint=np.ones(n, np.int32), nclass=np.ones(n, np.int32), idt=np.full(n, 1, np.int32),
                  uap=_uniform01(n, 80) - 0.5, xmass1=np.ones((nspec, n)) * 0.01)
    return rs


# --------------------------------------------------------------------------
# calcpar: the surface analysis it reads besides the model levels
# --------------------------------------------------------------------------
def calcpar_inputs(m, lsubgrid=1):
    """surfstr, sshf (both signs: stable and convective columns), excessoro and the half-level coefficients akm, bkm for a
    synthetic.model_levels() dict (compact [ny][nx] arrays)."""
    nx, ny, nz = (int(v) for v in m["grid"])
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, :]
    j = np.arange(ny, dtype=np.int64)[:, None]
    surfstr = 0.02 + 0.5 * (0.5 + 0.5 * _wave(3 * i + j, per)) ** 2 + 0.0 * j
    sshf = -180.0 * _wave(2 * i + 3 * j, per) + 15.0 * _wave(5 * i, per) + 0.0 * j      # W/m2, negative = upward (convective)
    sshf = np.where(np.abs(sshf) < 4.0, 0.0, sshf)                                        # some columns with zero heat flux
    exc = 250.0 * np.maximum(0.0, _wave(i + 2 * j, per)) + 0.0 * j
    for a in (surfstr, sshf, exc):
        a[:, nx - 1] = a[:, 0]
    ak, bk = np.asarray(m["akz"]), np.asarray(m["bkz"])
    akm = np.concatenate([[ak[0]], 0.5 * (ak[1:] + ak[:-1])])          # half levels between the full levels (akm(1) = surface)
    bkm = np.concatenate([[bk[0]], 0.5 * (bk[1:] + bk[:-1])])
    return dict(surfstr=surfstr, sshf=sshf, excessoro=exc, akm=akm, bkm=bkm, lsubgrid=int(lsubgrid))


def calcpar_gfs_inputs(m, lsubgrid=1):
    """What the NCEP branch of calcpar reads besides the pressure levels of a gfs_levels() dict: calcpar_inputs' surfstr, sshf
    and excessoro, and hmix -- the mixing height as readwind_gfs took it from the GRIB file.  It runs from below hmixmin
    (100 m) to above hmixmax (4500 m), so that both clamps of calcpar.f90:165-166 fire."""
    c = calcpar_inputs(m, lsubgrid)
    nx, ny, nz = (int(v) for v in m["grid"])
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, :]
    j = np.arange(ny, dtype=np.int64)[:, None]
    hmix = 2400.0 + 2500.0 * _wave(i + 3 * j, per) + 0.0 * j         # about -100 m ... 4900 m
    hmix[:, nx - 1] = hmix[:, 0]
    return dict(surfstr=c["surfstr"], sshf=c["sshf"], excessoro=c["excessoro"], hmix=hmix, lsubgrid=int(lsubgrid))


# --------------------------------------------------------------------------
# convective mixing (convmix.f90): soundings with and without CAPE
# --------------------------------------------------------------------------
def convection_case(nx=24, ny=16, nuvz=46, n=4000, ncalls=3, ldirect=1, lsynctime=900, seed=11, nest=False):
    """ECMWF-shaped input of the convection scheme on a small grid: hybrid half levels akm, bkm (akm(1) = surface) with
    the full levels akz, bkz between them (level 1 = surface), two time slots of ps, tt2, td2, tth, qvh [2][nuvz][ny][nx]
    whose soundings range from warm, moist and conditionally unstable (deep convection: most of the matrix is used)
    over shallow and marginal cases to dry or cold columns in which CONVECT leaves through each of its early exits;
    `n` particles between the ground and 16 km, a tenth of them not due, `ncalls` consecutive calls one lsynctime apart
    (the cloud-base mass flux cbaseflux relaxes from call to call).  nest=True adds one nested wind field of twice the
    resolution over the middle of the domain with soundings of its own (a wrong grid choice shows) and its own mass flux."""
    per = nx
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nuvz, dtype=np.float64)
    eta_h = np.exp(-3.3 * (k / float(nuvz - 1)) ** 1.25)                 # half levels: 1 ... about 0.037 (37 hPa)
    bkm = eta_h ** 1.6
    bkm[0] = 1.0
    akm = 101325.0 * (eta_h - bkm)
    akm[0] = 0.0
    akz = np.concatenate([[0.0], 0.5 * (akm[:-1] + akm[1:])])
    bkz = np.concatenate([[1.0], 0.5 * (bkm[:-1] + bkm[1:])])
    out = dict(akz=akz, bkz=bkz, akm=akm, bkm=bkm)
    def soundings(gnx, gny, shift, scale):
        """ps, tt2, td2 [2][gny][gnx], tth, qvh [2][nuvz][gny][gnx]; `scale` grid cells of this grid per mother cell."""
        gi = np.arange(gnx, dtype=np.int64)[None, None, :]
        gj = np.arange(gny, dtype=np.int64)[None, :, None]
        gper = per * scale
        res = {}
        for slot in range(2):
            ii = gi + 3 * slot * scale + shift
            warm = 0.5 + 0.5 * _wave(ii[0] + 2 * gj[0], gper)            # 0 ... 1: cold/dry ... warm/moist
            ps = 101300.0 + 600.0 * _wave(2 * ii[0] + gj[0], gper) - 14000.0 * np.maximum(0.0, _wave(3 * ii[0] + 5 * gj[0], 2 * gper)) ** 3
            p = akz[:, None, None] + bkz[:, None, None] * ps[None]
            z = -7600.0 * np.log(p / ps[None])
            tsfc = 271.0 + 31.0 * warm + 0.0 * ps
            lapse = 0.0055 + 0.0015 * warm
            tth = np.maximum(tsfc[None] - lapse[None] * z, 198.0 + 8.0 * warm[None]) + 0.4 * _wave(ii + gj + 3 * np.arange(nuvz)[:, None, None], gper)
            rh = (0.25 + 0.65 * warm[None]) * np.exp(-z / (5000.0 + 4000.0 * warm[None])) + 0.05
            tc = tth - 273.15
            es = 611.2 * np.exp(17.67 * tc / (tc + 243.5))
            qs = 0.622 * es / np.maximum(p - 0.378 * es, 1.0)
            qvh = np.minimum(rh, 0.98) * qs
            tt2 = tth[0] + 0.6
            td2 = tt2 - (2.0 + 14.0 * (1.0 - warm))
            res[slot] = (ps, tt2, td2, tth, qvh)
        return {key: np.stack([res[0][idx], res[1][idx]]) for idx, key in enumerate(("ps", "tt2", "td2", "tth", "qvh"))}

    out.update(soundings(nx, ny, 0, 1))
    if nest:
        ix0, jy0, ix1, jy1, fac = nx // 4, ny // 4, (2 * nx) // 3, (2 * ny) // 3, 2
        nxn, nyn = (ix1 - ix0) * fac + 1, (jy1 - jy0) * fac + 1
        sn = soundings(nxn, nyn, 5, fac)
        out.update({k + "n": v for k, v in sn.items()})
        gi = np.arange(nxn, dtype=np.int64)[None, :]
        gj = np.arange(nyn, dtype=np.int64)[:, None]
        warmn = 0.5 + 0.5 * _wave(gi + 5 + 2 * gj, per * fac)
        # xln, yln, xrn, yrn in mother grid units, xresoln, yresoln (gridcheck_nests.f90)
        out.update(nest=np.array([nxn, nyn], np.int32), nestgeom=np.array([ix0, jy0, ix1, jy1, fac, fac], np.float64), par_nxmax=721,
                   cbasefluxn=np.where(warmn > 0.5, 0.1 * warmn ** 2, 0.0))
    # a run in progress: the cloud-base mass flux of the warm columns has built up (it starts from zero in others)
    warm0 = 0.5 + 0.5 * _wave(i[0] + 2 * j[0], per)
    cb0 = np.where(warm0 > 0.55, 0.12 * warm0 ** 2, 0.0)
    u = [_splitmix64(n, seed + q).astype(np.float64) / 2.0 ** 64 for q in range(4)]
    # backward runs: lsynctime and the wind-field times carry the sign of ldirect (readcommand.f90:381-384, getfields.f90)
    out.update(grid=np.array([nx, ny, nuvz], np.int32), nconvlev=nuvz - 2, ldirect=int(ldirect), lsynctime=int(lsynctime) * int(ldirect),
               memtime=np.array([0, 10800 * int(ldirect)], np.int32), itimes=np.arange(ncalls, dtype=np.int32) * int(lsynctime) * int(ldirect),
               height_nz=19000.0, cbaseflux=cb0,
               xtra1=0.3 + u[0] * (nx - 1.6), ytra1=0.3 + u[1] * (ny - 1.6), ztra1=16000.0 * u[2] ** 1.5,
               due=(u[3][:, None] + 0.013 * np.arange(ncalls)[None, :]) % 1.0 > 0.1, npart=n)
    return out


def nconvlev_gfs(akz):
    """gridcheck_gfs.f90:513-517: the first level i <= nuvz-2 whose pressure akz(i) (bkz = 0) lies below 50 hPa; a loop that runs
    out leaves i = nuvz - 1.  The clamp to nconvlevmax - 1 (:518-522) is the host's compile-time size and is not applied here."""
    nuvz = len(akz)
    for i in range(1, nuvz - 1):
        if float(akz[i - 1]) < 5000.0:
            return i
    return nuvz - 1


def convection_case_gfs(nx=24, ny=16, nz=26, n=4000, ncalls=3, ldirect=1, lsynctime=900, seed=11, terrain=False, deep=False):
    """NCEP-GFS-shaped input of the convection scheme (convmix.f90:180-188): two time slots of ps, tt2, td2 and of the z-level
    fields tt, qv, pplev [2][nz][ny][nx], as verttransform_gfs leaves them.  The columns have the shape of the GFS pressure
    levels: pplev(.,.,k) = ps * GFS_PLEV_HPA[k] / 1000 hPa with a wave of a few tenths of a per cent on it, pplev(.,.,1) up to
    30 Pa below ps.  nuvz = nz, akz = the pressures of the levels, nconvlev as gridcheck_gfs.f90:513-517 computes it.  The
    soundings are those of convection_case() on these pressures -- deep convection over shallow and marginal cases -- with
    patches of cold columns (CONVECT's exit on tconv(nk) < 250), of columns without moisture (the same exit, qconv(nk) <= 0)
    and of very dry ones heated at the ground (its exit on the lifting condensation level); stable columns without a mass flux from before take the
    exit on the buoyancy at cloud base.  terrain: ps down to about 700 hPa.  The stratosphere warms with height, which keeps
    the deepest convection at nconvtop <= nconvlev; deep: an isothermal one instead, so that CONVECT's inb reaches nconvlev and
    nconvtop = nconvlev + 1 -- with nz = 26 that is nuvz - 1, and redist reads level nuvz, which no GFS run writes.  Particles, due flags, times and cbaseflux as in
    convection_case()."""
    if not 6 <= nz <= len(GFS_PLEV_HPA):
        raise ValueError("convection_case_gfs: 6 <= nz <= %d" % len(GFS_PLEV_HPA))
    per = nx
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    kk = np.arange(nz, dtype=np.int64)[:, None, None]
    akz = 100.0 * np.array(GFS_PLEV_HPA[:nz], np.float64)
    ratio = (akz / akz[0])[:, None, None]
    res = {}
    for slot in range(2):
        ii = i + 3 * slot
        warm = 0.5 + 0.5 * _wave(ii[0] + 2 * j[0], per)                  # 0 ... 1: cold/dry ... warm/moist
        ps = 101300.0 + 600.0 * _wave(2 * ii[0] + j[0], per) - (31000.0 if terrain else 14000.0) * np.maximum(0.0, _wave(3 * ii[0] + 5 * j[0], 2 * per)) ** 3
        p = ps[None] * ratio * (1.0 + 0.003 * _wave(ii + j + 2 * kk, per))
        p[0] = ps - 15.0 * (1.0 + _wave(ii[0] + 3 * j[0], per))
        z = -7600.0 * np.log(p / ps[None])
        tsfc = 271.0 + 31.0 * warm
        lapse = 0.0055 + 0.0015 * warm
        # a stratosphere that warms with height keeps the deepest convection below nconvlev (nconvtop <= nconvlev)
        tt = np.maximum(tsfc[None] - lapse[None] * z, 198.0 + 8.0 * warm[None] + (0.0 if deep else 0.0025) * np.maximum(z - 12000.0, 0.0)) + 0.4 * _wave(ii + j + 3 * kk, per)
        rh = (0.25 + 0.65 * warm[None]) * np.exp(-z / (5000.0 + 4000.0 * warm[None])) + 0.05
        cold = ((2 * ii[0] + j[0]) % 13 == 0)
        nomoist = ((ii[0] + 4 * j[0]) % 17 == 3)
        dry = ((ii[0] + 3 * j[0]) % 11 == 5) & ~nomoist
        tt = tt - 50.0 * cold[None]
        tt[0] += 3.0 * dry            # superadiabatic at the ground: hm has its minimum at level 2, the parcel starts at level 1
        tc = tt - 273.15
        es = 611.2 * np.exp(17.67 * tc / (tc + 243.5))
        qs = 0.622 * es / np.maximum(p - 0.378 * es, 1.0)
        qv = np.minimum(rh, 0.98) * qs * np.where(dry, 1.0e-5, 1.0)[None] * np.where(nomoist, 0.0, 1.0)[None]
        tt2 = tt[0] + 0.6
        td2 = tt2 - (2.0 + 14.0 * (1.0 - warm))
        res[slot] = (ps, tt2, td2, tt, qv, p)
    out = {key: np.stack([res[0][idx], res[1][idx]]) for idx, key in enumerate(("ps", "tt2", "td2", "tt", "qv", "pplev"))}
    warm0 = 0.5 + 0.5 * _wave(i[0] + 2 * j[0], per)
    cb0 = np.where(warm0 > 0.55, 0.12 * warm0 ** 2, 0.0)
    u = [_splitmix64(n, seed + q).astype(np.float64) / 2.0 ** 64 for q in range(4)]
    height = make_height(nz, top=80000.0 if nz >= 60 else 30000.0, lin=0.05 if nz >= 60 else 0.15)     # base_scenario's z levels
    out.update(akz=akz, grid=np.array([nx, ny, nz], np.int32), nconvlev=nconvlev_gfs(akz), ldirect=int(ldirect), lsynctime=int(lsynctime) * int(ldirect),
               memtime=np.array([0, 10800 * int(ldirect)], np.int32), itimes=np.arange(ncalls, dtype=np.int32) * int(lsynctime) * int(ldirect),
               height_nz=float(height[-1]), cbaseflux=cb0,
               xtra1=0.3 + u[0] * (nx - 1.6), ytra1=0.3 + u[1] * (ny - 1.6), ztra1=16000.0 * u[2] ** 1.5,
               due=(u[3][:, None] + 0.013 * np.arange(ncalls)[None, :]) % 1.0 > 0.1, npart=n)
    return out


# --------------------------------------------------------------------------
# getvdep (calcpar.f90:171-189): land use, resistance tables, the surface fields it reads
# --------------------------------------------------------------------------
GV_NUMCLASS, GV_NI, GV_MAXSPEC = 13, 11, 5          # par_mod.f90:211,225
GV_BDATE = 2458864.0                                # 15 January 2020, 0 UTC (juldate.f90)
# wind-field times [s] after bdate: 15 January 2020, 10 November 2020 3 UTC, 1 October 2019 6 UTC (a backward run).  The
# southern rows see the date half a year on (getvdep.f90:54-56), the tropical ones always summer: a winter date (season
# 4) always meets summer (1) on the other side, so it takes three dates to see all five seasonal categories.
GV_WFTIMES = (0, 300 * 86400 + 10800, -106 * 86400 + 21600)


def getvdep_tables(nx, ny, nspec, seed=4100):
    """The arrays of com_mod that getvdep and its callees read, in C order (the Fortran shapes transposed): xlanduse
    [numclass][ny][nx] (most classes absent from a column, fractions summing to one), z0 [numclass], ri, rac
    [numclass][5], rcl, rgs, rlu [numclass][5][maxspec], the species constants [maxspec] and vset, schmi, fract
    [ni][maxspec].  Species cycle through the four kinds getvdep distinguishes: a gas (reldiff > 0), an aerosol
    (density > 0), one with a constant deposition velocity (dryvel > 0) and an inert one."""
    nc, ni, ms = GV_NUMCLASS, GV_NI, GV_MAXSPEC
    assert nspec <= ms
    u = _uniform01(nc * ny * nx, seed).reshape(nc, ny, nx)
    xl = np.where(u > 0.7, u - 0.7, 0.0)
    tot = np.zeros((ny, nx))
    for j in range(nc):
        tot = tot + xl[j]
    xl = xl / np.where(tot > 0.0, tot, 1.0)
    z0 = np.array([0.7, 0.1, 0.1, 1.0, 1.0, 0.7, 1.0e-4, 2.0e-3, 0.15, 0.1, 0.1, 1.0e-3, 0.3])
    ur = _uniform01(5 * nc, seed + 1).reshape(nc, 5)
    ri = np.where(ur > 0.8, 9999.0, 60.0 + 800.0 * ur * ur)
    rac = 2000.0 * _uniform01(5 * nc, seed + 2).reshape(nc, 5) ** 2
    def res(k):
        v = _uniform01(ms * 5 * nc, seed + k).reshape(nc, 5, ms)
        return np.where(v > 0.85, 9999.0, 50.0 + 4000.0 * v * v)
    kind = np.arange(ms) % 4
    gas, aero, const = kind == 0, kind == 1, kind == 2
    step = 1.0 + 0.25 * (np.arange(ms) // 4)
    reldiff = np.where(gas, 1.6 * step, -9.9)
    rm = np.where(gas, 10.0 * (step - 1.0), 0.0)
    henry = np.where(gas, 1.0e5 * step, 0.0)
    f0 = np.where(gas, 0.1 * step, 0.0)
    density = np.where(aero, 1400.0 * step, -9.0)
    dryvel = np.where(const, 0.005 * step, -9.9)
    vs = np.array([1.0e-6, 3.0e-6, 1.0e-5, 3.0e-5, 1.0e-4, 3.0e-4, 1.0e-3, 3.0e-3, 1.0e-2, 2.0e-2, 5.0e-2])
    sm = np.array([1.0e-1, 6.0e-2, 3.0e-2, 1.5e-2, 8.0e-3, 4.0e-3, 2.0e-3, 1.0e-3, 5.0e-4, 2.5e-4, 1.0e-4])
    fr = np.array([1.0, 2.0, 4.0, 8.0, 12.0, 16.0, 12.0, 8.0, 4.0, 2.0, 1.0]) / 70.0
    on = np.where(aero, 1.0, 0.0)[None, :]
    return dict(numclass=nc, ni=ni, maxspec=ms, nspec=int(nspec), bdate=GV_BDATE, xlanduse=xl, z0=z0, ri=ri, rac=rac,
                rcl=res(3), rgs=res(4), rlu=res(5), rm=rm, reldiff=reldiff, henry=henry, f0=f0, density=density, dryvel=dryvel,
                vset=vs[:, None] * step[None, :] * on, schmi=sm[:, None] / step[None, :] * on, fract=fr[:, None] * on)


def getvdep_inputs(m_or_shape, seed=4200, wftime=0):
    """ssr, lsprec, convprec, sd (compact [ny][nx]) for fpx_getvdep: radiation from night to noon, a quarter of the columns
    with rain, an eighth under snow.  Given a shape (ny, nx) instead of a synthetic.model_levels() dict, also the fields
    the device would otherwise take from fpx_calcpar and the transform: ustar (a few columns at calcpar's floor of
    1e-8), oli (both signs, |L| = 9999 among them), ps, tt2 (from -35 to +50 C), td2 (a fifth of the columns above 90 %
    relative humidity)."""
    full = not isinstance(m_or_shape, dict)
    ny, nx = (int(v) for v in m_or_shape) if full else (int(m_or_shape["grid"][1]), int(m_or_shape["grid"][0]))
    u = [_uniform01(ny * nx, seed + k).reshape(ny, nx) for k in range(11)]
    out = dict(wftime=int(wftime),
               ssr=np.maximum(0.0, 900.0 * u[0] - 100.0),
               lsprec=np.where(u[1] > 0.8, 3.0 * (u[1] - 0.8), 0.0),
               convprec=np.where(u[2] > 0.9, 5.0 * (u[2] - 0.9), 0.0),
               sd=np.where(u[3] > 0.85, 0.05 * (u[3] - 0.85), 0.0))
    if full:
        ol = np.where(u[5] < 0.5, 1.0, -1.0) * (5.0 + 2000.0 * u[6] * u[6])
        ol = np.where(u[5] < 0.06, 9999.0, np.where(u[5] > 0.94, -9999.0, ol))
        tt2 = 273.15 + (85.0 * u[8] - 35.0)
        out.update(ustar=np.where(u[4] < 0.03, 1.0e-8, 0.05 + 0.9 * u[4] * u[4]), oli=1.0 / ol,
                   ps=60000.0 + 45000.0 * u[7], tt2=tt2, td2=tt2 - 30.0 * u[9] * u[9])
    return out


# --------------------------------------------------------------------------
# calcpar_nests / getvdep_nests: the same inputs on a nested grid (a nest_model_levels() dict), with patterns and draws of
# their own, so that a mother-grid array read in a nest's place shows
# --------------------------------------------------------------------------
def nest_calcpar_inputs(n, lsubgrid=1):
    """surfstrn, sshfn, excessoron (compact [nyn][nxn]) and akm, bkm for a nest_model_levels() dict, under the keys of
    calcpar_inputs()."""
    c = calcpar_inputs(n, lsubgrid)
    c["surfstr"] = c["surfstr"][::-1, :].copy() * 1.25
    c["sshf"] = -c["sshf"][:, ::-1].copy()
    c["excessoro"] = c["excessoro"][::-1, ::-1].copy()
    return c


def nest_getvdep_tables(n, nspec, seed=4150):
    """getvdep_tables() whose xlanduse is the nest's xlandusen(:,:,:,l), [numclass][nyn][nxn]; the small tables are the
    mother grid's (com_mod has one set)."""
    return getvdep_tables(int(n["grid"][0]), int(n["grid"][1]), nspec, seed=seed)


def nest_getvdep_inputs(n_or_shape, seed=4250, wftime=0):
    """getvdep_inputs() on a nest: ssrn, lsprecn, convprecn, sdn (and, given a shape (nyn, nxn), ustarn, olin, psn, tt2n, td2n)."""
    return getvdep_inputs(n_or_shape, seed=seed, wftime=wftime)


def no_tropopause_columns(n, mask):
    """A copy of a model_levels() / nest_model_levels() dict in which the columns `mask` [ny][nx] cool by more than 2 K/km
    all the way to the model top, free of isothermal or inversion layers: no layer meets the thermal-tropopause criterion
    (calcpar.f90:236-258, calcpar_nests.f90:201-214) there, so the tropopause of such a column keeps its previous value."""
    out = dict(n)
    ak, bk, ps = np.asarray(n["akz"]), np.asarray(n["bkz"]), np.asarray(n["ps"])
    zapprox = -7400.0 * np.log((ak[:, None, None] + bk[:, None, None] * ps[None]) / 101325.0)
    out["tth"] = np.where(np.asarray(mask)[None], 300.0 - 0.0030 * zapprox, np.asarray(n["tth"]))
    return out


# --------------------------------------------------------------------------
# calcpv / calcpv_nests: model-level input that drives every branch of the theta-surface search
# --------------------------------------------------------------------------
PV_NX, PV_NY, PV_NZ = 37, 29, 20           # nlck = nuvz/3 = 6: searches do run out
PV_NXMAX, PV_NYMAX = 40, 32                # the strides of the host's arrays differ from the extents
PV_CASES = ("limited", "global", "nest")
PV_GEOM = {"limited": (1.0, 0.75, -20.0, 20.5),                         # dx, dy, xlon0, ylat0
           "global": (360.0 / (PV_NX - 1), 180.0 / (PV_NY - 1), -180.0, -90.0),
           "nest": (0.25, 0.2, -10.0, 30.1)}                            # dxn, dyn, xlon0n, ylat0n inside the 'limited' grid
PV_HOT = ((20, 12), (21, 12), (22, 12), (20, 13), (21, 13), (22, 13), (20, 14), (21, 14), (22, 14),   # a 3 x 3 block ...
          (28, 20), (30, 8), (0, 15), (14, 0))                          # ... and single columns, two of them on an edge
PV_TIES = ((8, 18, 6), (25, 6, 9), (16, 22, 3))                         # (ix, jy, kl 1-based): theta met within 4e-6 K next door
PV_TIE_REL = 6.0e-9


def _ln_series(x):
    """ln x for x near 1 from +, *, / alone (2 atanh((x-1)/(x+1))): the same bits on every platform."""
    z = (x - 1.0) / (x + 1.0)
    z2, t, acc = z * z, z, 0.0
    for n in range(40):
        acc = acc + t / float(2 * n + 1)
        t = t * z2
    return 2.0 * acc


def _exp_series(y):
    t, acc = 1.0, 1.0
    for n in range(1, 40):
        t = t * y / float(n)
        acc = acc + t
    return acc


def _hash01(shape, seed):
    return _uniform01(int(np.prod(shape)), seed).reshape(shape)


def calcpv_case(name):
    """Model-level input of one of the three cases of tests/golden/pv_r*.npz as compact [nz][ny][nx] float64 arrays, from
    integer hashes and IEEE-exact operations only (+, -, *, /, comparisons, rounding to a binary fraction), so that the
    tests regenerate the fixture's inputs bit for bit.  Besides what calcpv reads (akz, bkz, ps, tth, uuh, vvh) the dict
    has everything fpx_verttransform_ecmwf needs (wwh, qvh, tt2, td2, aknew, bknew, an arbitrary pvh) and grid, geom,
    globalflags.  The temperature has
      * noise and a patch with a warm level 2 and a cold level 4: theta inversions near the ground, which put a bracket
        below the level searched from and give non-adjacent brackets;
      * columns 150 K warmer than their neighbours at all levels (PV_HOT): their theta is not met next door within six
        levels, and theirs is not met from next door -- no bracket on one side (next to the block, on its rim) and on
        both (the single columns);
      * three columns (PV_TIES, ix + 1) whose levels kl, kl + 1 bracket the theta of (ix, jy, kl) within 6e-9 relative
        on either side: dt = dt1 + dt2 < eps in r8 (calcpv.f90:153), each endpoint 6e-9 away from its own decision.
    'global' carries the duplicated meridian (column nx-1 = column 0) and sets xglobal, nglobal, sglobal; 'nest' is the
    input of calcpv_nests: the same arrays on the nest's geometry (dxn != dyn, its own ylat0n)."""
    if name not in PV_CASES:
        raise ValueError(name)
    nx, ny, nz = PV_NX, PV_NY, PV_NZ
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    s = np.arange(ny, dtype=np.float64)[None, :, None] / float(ny - 1)
    clat = 4.0 * s * (1.0 - s)
    q = 1.0 - np.arange(nz, dtype=np.float64) / float(nz - 1)
    eta = 0.002 + 0.998 * q * q
    eta[0] = 1.0
    bk = eta * eta
    ak = 101325.0 * (eta - bk)
    ak[0] = 0.0
    mount = np.maximum(0.0, _wave(2 * i[0] + 3 * j[0], per)) * np.maximum(0.0, _wave(3 * j[0] + 7, 2 * (ny - 1)))
    ps = np.rint((101200.0 + 900.0 * _wave(i[0] + 2 * j[0], per) - 30000.0 * mount * mount) * 8.0) / 8.0
    for ix, jy, _ in PV_TIES:
        ps[jy, ix + 1] = ps[jy, ix]
    p3 = ak[:, None, None] + bk[:, None, None] * ps[None]
    rel = p3 / 101325.0
    base = np.maximum(288.0 - 80.0 * (1.0 - rel), 216.0) + 2.0 * _wave(i + j + 2 * k, per) + 6.0 * (clat - 0.5)
    tth = base + 1.5 * (_hash01((nz, ny, nx), 7100) - 0.5)
    tth[1, 4:11, 5:13] += 6.0
    tth[3, 4:11, 5:13] -= 5.0
    tth = np.rint(tth * 1024.0) / 1024.0
    for ix, jy in PV_HOT:
        tth[:, jy, ix] += 150.0
    for ix, jy, kl in PV_TIES:
        # theta(ix+1, kl) = theta(ix, kl) (1 + d): same ps, same level, so the same ppmk; theta(ix+1, kl+1) = theta(ix, kl) (1 - d)
        # through the ratio of the two levels' (100000/p)**kappa, from the series above (accurate to 1e-15, far inside d)
        r = _exp_series(0.286 * _ln_series(float(p3[kl, jy, ix]) / float(p3[kl - 1, jy, ix])))
        tth[kl - 1, jy, ix + 1] = tth[kl - 1, jy, ix] * (1.0 + PV_TIE_REL)
        tth[kl, jy, ix + 1] = tth[kl - 1, jy, ix] * r * (1.0 - PV_TIE_REL)
    uuh = np.rint((22.0 * clat * (1.0 + 0.3 * _wave(k, nz)) + 6.0 * _wave(3 * i, per) + 0.0 * j + 3.0 * (_hash01((nz, ny, nx), 7200) - 0.5)) * 64.0) / 64.0
    vvh = np.rint((6.0 * _wave(2 * i + 0 * j, per) * clat + 2.0 * _wave(k + 3 * j, 40) + 3.0 * (_hash01((nz, ny, nx), 7300) - 0.5)) * 64.0) / 64.0
    qvh = 0.012 * rel * rel * rel * (0.6 + 0.4 * _wave(2 * i + j, per))
    wwh = 0.4 * _wave(i, per) * _wave(2 * j + 0 * i, ny - 1) * rel
    pvh = 1.0e-6 * (1.0 + 0.5 * _wave(i + k, per)) * (2.0 * s - 1.0) / (rel + 0.05)
    tt2 = base[0] + 0.5 * _wave(3 * i[0] + j[0], per)
    td2 = tt2 - 3.0 - 2.0 * (1.0 + _wave(i[0] + 5 * j[0], per))
    out = dict(akz=ak, bkz=bk, aknew=ak.copy(), bknew=bk.copy(), ps=ps, tt2=tt2, td2=td2, tth=tth, qvh=qvh, uuh=uuh, vvh=vvh,
               pvh=pvh, wwh=wwh)
    glob = name == "global"
    if glob:
        for key in ("ps", "tt2", "td2", "tth", "qvh", "uuh", "vvh", "pvh", "wwh"):
            out[key][..., nx - 1] = out[key][..., 0]
    out["grid"] = np.array([nx, ny, nz], np.int32)
    out["geom"] = np.array(PV_GEOM[name], np.float64)
    out["globalflags"] = np.array([int(glob)] * 3, np.int32)
    return out


# --------------------------------------------------------------------------
# calcfluxes / fluxoutput (tests/golden/cf_r*.npz)
# --------------------------------------------------------------------------
CF_VARIANTS = ("release", "domainfill")


def calcfluxes_case(variant="release"):
    """Prepared particles for the reference's calcfluxes and fluxoutput, from integer hashes and IEEE-exact operations
    only, so that the tests regenerate the fixture's inputs bit for bit.  Met grid 20 x 12 (dx 1, dy 0.5), output grid
    6 x 4 x 3 with cells of 0.3 x 0.2 degrees whose origin lies inside the met grid (particles lie west and south of
    it), 2 species, 3 release points with ioutputforeachrelease = 1, 2 age classes.  `ncalls` batches of particles, each
    with a position before (xold.. as the double / real the particle arrays held) and after the move; masses are small
    integers times 2**-10, so every sum is exact in either real kind and in any order.  The last eight particles of a
    batch move by more than nx/2 (the cyclic branch, both directions).  'domainfill' is a small second case with
    mdomainfill = 1 and npoint = the particle number, as a domain-filling run has it: kp = 1 for every particle."""
    if variant not in CF_VARIANTS:
        raise ValueError(variant)
    fill = variant == "domainfill"
    n, ncalls = (60, 1) if fill else (300, 2)
    nspec, numpoint = 2, 3
    c = dict(grid=np.array([20, 12], np.int32), geom=np.array([1.0, 0.5, -10.0, 40.0], np.float64),
             outgrid=np.array([6, 4, 3], np.int32), outgeom=np.array([0.3, 0.2, -3.7, 42.1], np.float64),
             outheight=np.array([100.0, 500.0, 1500.0], np.float64), nspec=nspec, numpoint=numpoint,
             ioutputforeachrelease=1, mdomainfill=int(fill), maxpointspec_act=numpoint, lage=np.array([3600, 86400], np.int32),
             itime=10800, bdate=2458864.0, outstep=3600.0, ncalls=ncalls, npart=n)
    nxg, nyg, nzg = (int(v) for v in c["outgrid"])
    # wall areas: any positive numbers do (fluxoutput only divides by them); dyadic fractions of 1e8, exact in both kinds
    c["area"] = 1.0e8 * (1.0 + np.floor(_hash01((nyg, nxg), 8100) * 64.0) / 64.0)
    c["areaeast"] = 1.0e6 * (1.0 + np.floor(_hash01((nzg, nyg, nxg), 8200) * 64.0) / 64.0)
    c["areanorth"] = 1.0e6 * (1.0 + np.floor(_hash01((nzg, nyg, nxg), 8300) * 64.0) / 64.0)
    for b in range(ncalls):
        s = 9000 + 100 * b + (50 if fill else 0)
        xo = 5.3 + 3.8 * _uniform01(n, s + 1)
        yo = 3.6 + 2.8 * _uniform01(n, s + 2)
        zo = 2000.0 * _uniform01(n, s + 3)
        xn = xo + 2.4 * (_uniform01(n, s + 4) - 0.5)
        yn = yo + 1.6 * (_uniform01(n, s + 5) - 0.5)
        zn = 2000.0 * _uniform01(n, s + 6)
        still = np.arange(n) % 7 == 3                        # some stay on their level, some in their column
        zn[still] = zo[still] + 20.0 * (_uniform01(n, s + 7)[still] - 0.5)
        zn = np.abs(zn)
        cyc = np.arange(n) >= n - 8
        east = cyc & (np.arange(n) % 2 == 0)
        xo[cyc] = np.where(east[cyc], 0.4, 18.7) + 0.5 * _uniform01(n, s + 8)[cyc]
        xn[cyc] = np.where(east[cyc], 18.6, 0.3) + 0.5 * _uniform01(n, s + 9)[cyc]
        yo[cyc] = 4.4 + 1.2 * _uniform01(n, s + 10)[cyc]
        yn[cyc] = yo[cyc] + 0.2
        zo[cyc] = zn[cyc] = 200.0
        h = _splitmix64(n, s + 11)
        m = np.zeros((nspec, n), np.float64)
        m[0] = (1 + (h % np.uint64(8)).astype(np.int64)).astype(np.float64) / 1024.0
        second = (h >> np.uint64(8)) % np.uint64(6) == np.uint64(0)
        age = ((h >> np.uint64(24)) % np.uint64(5000)).astype(np.int64)          # most in the first age class
        second = second | (age >= 3600)                                          # the second species: one in six, and every old particle
        m[1] = np.where(second, (1 + ((h >> np.uint64(16)) % np.uint64(4)).astype(np.int64)).astype(np.float64) / 1024.0, 0.0)
        old = (h >> np.uint64(40)) % np.uint64(16) == np.uint64(0)                # the few of the second class sit in one corner
        age[old] += 3600
        xo[old & ~cyc] = 6.4 + 0.25 * _uniform01(n, s + 12)[old & ~cyc]
        xn[old & ~cyc] = xo[old & ~cyc] + 0.35
        c[f"xold{b}"], c[f"yold{b}"], c[f"zold{b}"] = xo, yo, zo
        c[f"xnew{b}"], c[f"ynew{b}"], c[f"znew{b}"] = xn, yn, zn
        c[f"xmass1_{b}"] = m
        c[f"npoint{b}"] = (np.arange(n) + 1).astype(np.int32) if fill else (1 + ((h >> np.uint64(48)) % np.uint64(numpoint)).astype(np.int64)).astype(np.int32)
        c[f"itramem{b}"] = (int(c["itime"]) - age).astype(np.int32)
    return c


# --------------------------------------------------------------------------
# partpos_average / partoutput_average (tests/golden/pa_r*.npz)
# --------------------------------------------------------------------------
PA_SUMS = ("cartx", "carty", "cartz", "z", "topo", "pv", "qv", "tt", "uu", "vv", "rho", "tro", "hmix", "energy")


def partavg_case():
    """Prepared particles for the reference's partpos_average and partoutput_average, from integer hashes and IEEE-exact
    operations only, so that the tests regenerate the fixture's inputs bit for bit.  Met grid 20 x 12 x 10 with dx = 10,
    dy = 4 degrees from (-9.9999998, -4) -- longitudes -10 .. 180, latitudes -4 .. 40 -- and nymax = ny; the wind-field window is
    0 .. 10800 s with memind = (2, 1).  Two output intervals: six calls (itime 900 .. 5400) and the output at 6300, three
    more calls (6300 .. 8100) and the output at 9000.  Per call every particle has a position and a flag whether the
    particle loop reaches it (itra1 = itime); per output an itra1.  240 particles, by j % 8:
      5     moved in the first three calls only and terminated afterwards: a hole in both files (so are the last three
            particles: the files end before them);
      6     released before the fourth call: npart_av = 3 at the first output;
      3     (the first ten of them) inside two columns with extreme values -- qv 0.07, pv +-400, uu 180, vv -170 and, on the
            two top levels, tt 150 K in the south and 330 K in the north -- half of them above 70 km: the clamps of z, qv,
            pv, tt, uu, vv and energy;
      else  a cloud over lon -8 .. 10, lat -3 .. 38, drifting from call to call.
    Particles 1 and 9 sit on the northern boundary row (yt = ny - 1: the jyp >= nymax fix-up), particles 2 and 10 at
    longitude 180.0000001 in an 8-byte build: the angle goes to radians and back with the same pi180, so the result exceeds
    180 -- the wrap of partoutput_average.f90:103 -- only for a longitude in the sliver between 180 and pi / pi180 =
    180.0000002 (the pi of par_mod is a little short).  A 4-byte real cannot reach the wrap at all: xlon0 and the longitude
    round to -10 and 180, and the largest atan2(..) / pi180, 180.000006, rounds to 180.0."""
    nx, ny, nz, n = 20, 12, 10, 240
    height = make_height(nz)
    f = make_fields(nx, ny, nz, height)
    c = dict(grid=np.array([nx, ny, nz], np.int32), geom=np.array([10.0, 4.0, -9.9999998, -4.0], np.float64), nymax=ny, height=height,
             memtime=np.array([0, 10800], np.int32), memind=np.array([2, 1], np.int32), bdate=GV_BDATE, npart=n,
             calls=((900, 1800, 2700, 3600, 4500, 5400), (6300, 7200, 8100)), outputs=(6300, 9000))
    per = nx - 1
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    z = height[:, None, None]
    oro = 400.0 * (1.0 + _wave(2 * i[0] + 3 * j[0], per)) + 0.0 * j[0]
    pv = np.empty((2, nz, ny, nx)); qv = np.empty((2, nz, ny, nx))
    for m in range(2):
        sh = 10 * m
        pv[m] = 2.0 * (1.0 + 0.5 * _wave(i + sh + k, per)) * (1.0 + z / 6000.0) * (2.0 * j / float(ny - 1) - 1.0)
        qv[m] = 0.012 / (1.0 + z / 2500.0) ** 2 * (0.6 + 0.4 * _wave(2 * (i + sh) + j, per)) + 0.0 * k
    uu, vv, tt = f["uu"].copy(), f["vv"].copy(), f["tt"].copy()
    hot = slice(3, 5)                                    # columns 3 and 4: longitudes 20 and 30
    qv[..., hot] = 0.07
    pv[:, :, :6, hot] = 400.0
    pv[:, :, 6:, hot] = -400.0
    uu[..., hot] = 180.0
    vv[..., hot] = -170.0
    tt[:, nz - 2:, :6, hot] = 150.0
    tt[:, nz - 2:, 6:, hot] = 330.0
    for key, a in (("oro", oro), ("pv", pv), ("qv", qv), ("tt", tt), ("uu", uu), ("vv", vv), ("rho", f["rho"]),
                   ("tropopause", f["tropopause"]), ("hmix", f["hmix"])):
        c[key] = a
    idx = np.arange(n)
    cls = idx % 8
    cls[n - 3:] = 5
    extreme = (cls == 3) & (idx < 80)
    x0 = 0.2 + 1.8 * _uniform01(n, 9501)
    y0 = 0.3 + 10.0 * _uniform01(n, 9502)
    z0 = 30.0 + 11000.0 * _uniform01(n, 9503) ** 2
    x0[extreme] = 3.05 + 0.9 * _uniform01(n, 9504)[extreme]
    z0[extreme & (idx % 16 == 3)] = 70000.0 + 9000.0 * _uniform01(n, 9505)[extreme & (idx % 16 == 3)]
    ncall = 0
    for iv, times in enumerate(c["calls"]):
        for itime in times:
            s = 9600 + 20 * ncall
            xt = x0 + 0.02 * ncall + 0.03 * (_uniform01(n, s + 1) - 0.5)
            yt = y0 + 0.015 * ncall + 0.03 * (_uniform01(n, s + 2) - 0.5)
            zt = np.abs(z0 + 40.0 * (_uniform01(n, s + 3) - 0.5))
            xt[extreme] = np.minimum(xt[extreme], 3.98)
            yt[[1, 9]] = float(ny - 1)
            xt[[2, 10]] = 18.99999999
            due = np.ones(n, bool)
            due[cls == 5] = ncall < 3
            due[cls == 6] = ncall >= 3
            c[f"xt{ncall}"], c[f"yt{ncall}"], c[f"zt{ncall}"], c[f"due{ncall}"] = xt, yt, zt, due.astype(np.int32)
            ncall += 1
        itra1 = np.full(n, c["outputs"][iv], np.int32)
        itra1[cls == 5] = DEAD
        c[f"itra1_{iv}"] = itra1
    c["ncalls"] = ncall
    return c


# --------------------------------------------------------------------------
# initial_cond_calc / initial_cond_output (tests/golden/ic_r*.npz)
# --------------------------------------------------------------------------
IC_VARIANTS = ("mass", "mixing", "points", "domainfill")


def initcond_case(variant="mass"):
    """Prepared particles for the reference's initial_cond_calc and initial_cond_output, from integer hashes and IEEE-exact
    operations only, so that the tests regenerate the fixture's inputs bit for bit.  Met grid 20 x 12 x 10 (dx 1, dy 0.5
    from (-10, 40)), memind = (2, 1): the second wind field in memory is the physical slot 1.  Output grid 12 x 8 x 3 of
    quarter cells with its origin at met (7.5, 4.0): xl = 4 xt - 30, yl = 4 yt - 16, exact in both real kinds.  300
    particles over xl -1.2 .. 12.9, yl -0.7 .. 8.6 -- outside on all four sides -- with a band xl 5.1 .. 6.9 left empty so
    that the rows of the grid have holes; heights up to 2000 m (the top output level is 1500 m); every seventh particle is
    not due (itra1 differs from itime).  The first four particles sit at xl = 0.5 and at yl = 0.5 exactly: the uniform
    kernel then looks at column -1 / row -1 (the only neighbours outside the grid it can ever look at: beyond
    numxgrid - 1.5 the direct attribution takes over).
      mass        linit_cond = 1, one species, one release index
      mixing      linit_cond = 2, the same particles
      points      linit_cond = 1, ioutputforeachrelease = 1, three release points, two species, ind_rel = 1 with a rho_rel
      domainfill  linit_cond = 2, mdomainfill = 1, npoint = the particle number: nrelpointer = 1 all the same"""
    if variant not in IC_VARIANTS:
        raise ValueError(variant)
    nx, ny, nz, n = 20, 12, 10, 300
    points, fill = variant == "points", variant == "domainfill"
    nspec = 2 if points else 1
    mps = 3 if points else 1
    height = make_height(nz)
    f = make_fields(nx, ny, nz, height)
    c = dict(grid=np.array([nx, ny, nz], np.int32), geom=np.array([1.0, 0.5, -10.0, 40.0], np.float64), height=height,
             memind=np.array([2, 1], np.int32), rho=f["rho"],
             outgrid=np.array([12, 8, 3], np.int32), outgeom=np.array([0.25, 0.125, -2.5, 42.0], np.float64),
             outheight=np.array([100.0, 500.0, 1500.0], np.float64), nspec=nspec, maxpointspec_act=mps,
             ioutputforeachrelease=int(points), mdomainfill=int(fill), linit_cond=1 if variant in ("mass", "points") else 2,
             ind_rel=int(points), itime=-10800, npart=n)
    s = 9800 + 10 * IC_VARIANTS.index(variant if variant != "mixing" else "mass")
    xl = -1.2 + 14.1 * _uniform01(n, s + 1)
    band = (xl > 5.1) & (xl < 6.9)
    xl[band] = xl[band] + 1.8
    yl = -0.7 + 9.3 * _uniform01(n, s + 2)
    xt = (np.floor(xl * 4096.0) / 4096.0 + 30.0) / 4.0
    yt = (np.floor(yl * 4096.0) / 4096.0 + 16.0) / 4.0
    zt = 2000.0 * _uniform01(n, s + 3) ** 2
    xt[0], yt[0] = 7.625, 4.6                            # xl = 0.5: ixp = -1
    xt[1], yt[1] = 7.625, 5.3
    xt[2], yt[2] = 8.4, 4.125                            # yl = 0.5: jyp = -1
    xt[3], yt[3] = 9.7, 4.125
    zt[:4] = (40.0, 300.0, 900.0, 60.0)
    h = _splitmix64(n, s + 4)
    m = np.zeros((nspec, n), np.float64)
    m[0] = (1.0 + (h % np.uint64(1000)).astype(np.float64)) / 3000.0
    if nspec > 1:
        m[1] = (1.0 + ((h >> np.uint64(16)) % np.uint64(1000)).astype(np.float64)) / 7000.0
    itra1 = np.full(n, c["itime"], np.int32)
    idx = np.arange(n)
    itra1[idx % 7 == 5] = c["itime"] + 900
    itra1[idx % 31 == 11] = DEAD
    c["xtra1"], c["ytra1"], c["ztra1"], c["xmass1"], c["itra1"] = xt, yt, zt, m, itra1
    c["npoint"] = (idx + 1).astype(np.int32) if fill else (1 + ((h >> np.uint64(48)) % np.uint64(mps)).astype(np.int64)).astype(np.int32)
    c["xmass"] = np.array([[1.0, 2.5, 0.75], [0.5, 4.0, 1.25]][:nspec], np.float64)[:, :mps]      # [nspec][numpoint]
    c["rho_rel"] = np.array([1.125, 0.9375, 1.0625][:mps], np.float64)
    return c


PT_VARIANTS = ("blobs", "diffuse")
PT_NCLUSTER = 5
# per release point: live particles (multiples of 5 where the point is clustered), ireleasestart, ireleaseend
PT_POINTS = ((2380, -1800, 0), (300, -60000, -58200), (0, -900, 1), (3, -3600, -1801), (5, 0, 900), (600, -7200, -3600), (600, -5400, -2700))
PT_CENTRES = ((-8.0, 3.5), (6.0, -5.0), (0.0, 0.0), (11.0, 6.0), (0.0, 0.0), (7.0, 4.5), (0.0, 0.0))   # lon, lat of the points
PT_OFFSETS = ((-5.0, -3.0), (-5.0, 3.0), (0.0, 0.0), (5.0, -3.0), (5.0, 3.0))                           # of a point's five groups


def _pt_lattice(nxl, nyl, step, last, hollow):
    """A symmetric nxl x nyl lattice of offsets (degrees) around (0, 0), row by row, without the offsets closer than `hollow`
    to the centre in both directions, and with the offset `last` ('centre', kept then, or 'corner') moved to the end: the
    k-means takes its seeds from the ends of the fifths of a point's list."""
    ox = (np.arange(nxl) - (nxl - 1) / 2.0) * step
    oy = (np.arange(nyl) - (nyl - 1) / 2.0) * step
    gx, gy = np.meshgrid(ox, oy)
    gx, gy = gx.ravel(), gy.ravel()
    centre = (gx == 0.0) & (gy == 0.0)
    keep = ~((np.abs(gx) < hollow) & (np.abs(gy) < hollow)) | (centre & (last == "centre"))
    gx, gy = gx[keep], gy[keep]
    k = int(np.nonzero((gx == 0.0) & (gy == 0.0))[0][0]) if last == "centre" else gx.size - 1
    order = np.r_[np.delete(np.arange(gx.size), k), k]
    return gx[order], gy[order]


def plumetraj_case(variant="blobs"):
    """A scenario for plumetraj.f90 / clustering.f90 (iout = 4, 5): small(nx=40, ny=24, nz=30) as a limited-area grid of one
    degree from (-20, -12), so that both hemispheres are present, with oro, pv, qv of add_partoutput_fields, the PV scaled
    to pvu and signed like the latitude (|PV| passes 2 near 6 km).  Every seventh particle is terminated; the live ones
    belong to seven release points (PT_POINTS) and six to none (npoint 0 and 8).  Point 1 has 2380 particles (three chunks
    of 1024), point 2 is too old at itime = 0 (lage = 20000 s), point 3 has no particle, point 4 three (fewer than
    clusters), point 5 exactly five, points 6 and 7 600 each.  The particles of the points lie interleaved in storage; the
    order within a point is what counts.  Heights cycle through 50 m .. 14 km: both sides of hmix, of the tropopause and of
    |PV| = 2.
      blobs    every point's particles lie on symmetric lattices of 0.05 degrees around five group centres several degrees
               apart, stored group by group in equal numbers, each group ending with a corner of its lattice: the five seeds
               fall into five groups, pass 2 moves the centroids to the groups' centres and pass 3 repeats pass 2 bit for
               bit (the ratio of the exit test is exactly 0, whatever the order of the sums).  The lattices are hollow: no
               particle lies within 0.2 degrees of its group's centre, i.e. near the edge of distance2's box around a
               centroid that carries a summation error.
      diffuse  one wide cloud of several degrees per point: many passes, bisectors through the cloud.  Point 6 ends its fourth
               and fifth fifth with one and the same position: two equal seeds, cluster 5 is empty in pass 1.  Point 7 (605
               particles here) keeps lattices, each ending with its centre: the seeds are the groups' centres and the loop
               is left in pass 2.
    In both, point 5's five particles lie within a degree of (0, 0), where longitude and latitude in radians are small and the
    relative errors of sin, cos and atan2 leave them accurate to 1e-8 rad even in r4: each is its own seed and its own centroid
    (distance2's box in every pass: rms = 0, the exit test is 0/0 and never true, 100 passes), and the centre of mass falls on the
    middle one (distance's 0.03 degree box)."""
    if variant not in PT_VARIANTS:
        raise ValueError(variant)
    points = [list(p) for p in PT_POINTS]
    if variant == "diffuse":
        points[6][0] = 605
    nlive = sum(p[0] for p in points) + 6
    n = (7 * nlive + 5) // 6
    assert n - (n + 6) // 7 == nlive
    sc = small(n=n, nx=40, ny=24, nz=30, nsteps=1, global_grid=False, seed=770)
    sc["geom"] = np.array([1.0, 1.0, -20.0, -12.0], np.float64)
    add_partoutput_fields(sc, itime=0)
    ny = 24
    lat = -12.0 + np.arange(ny, dtype=np.float64)
    sign = np.where(lat > 0.0, 1.0, -1.0)[None, None, :, None]
    sc["pv"] = np.abs(sc["pv"]) * 2.0e6 * sign
    numpoint = len(points)
    sc["numpoint"] = numpoint
    sc["xmass"] = np.ones((1, numpoint), np.float64)
    sc["npart_rel"] = np.full(numpoint, 1000, np.int32)
    sc["lage"] = np.array([20000], np.int32)
    sc["ireleasestart"] = np.array([p[1] for p in points], np.int32)
    sc["ireleaseend"] = np.array([p[2] for p in points], np.int32)
    # labels of the live particles: the multiset of the points, interleaved by a hash, the order within a point kept
    lab = np.concatenate([np.full(p[0], j + 1, np.int64) for j, p in enumerate(points)] + [np.array([0, 8, 0, 8, 0, 8], np.int64)])
    lab = lab[np.argsort(_splitmix64(nlive, 0x9717), kind="stable")]
    lon = np.zeros(nlive); la = np.zeros(nlive)
    u1, u2 = _uniform01(nlive, 0x9718), _uniform01(nlive, 0x9719)
    for j, (cnt, _, _) in enumerate(points):
        who = np.nonzero(lab == j + 1)[0]
        if cnt == 0:
            continue
        cx, cy = PT_CENTRES[j]
        lattice = cnt >= 5 and j != 1 and (variant == "blobs" or j == 6)
        if not lattice:
            # a wide cloud: +-4 degrees by +-2.5 (the small points: their first particles)
            lon[who] = cx + 8.0 * (u1[who] - 0.5); la[who] = cy + 5.0 * (u2[who] - 0.5)
            if j == 5:                                  # point 6: the fourth and the fifth seed are one and the same position
                lon[who[cnt - 1]] = lon[who[4 * cnt // 5 - 1]]; la[who[cnt - 1]] = la[who[4 * cnt // 5 - 1]]
            continue
        m = cnt // 5
        if cnt == 5:                                    # point 5: (0, 0) and four positions less than a degree from it
            lon[who] = np.array([-0.8, -0.8, 0.0, 0.8, 0.8]); la[who] = np.array([-0.5, 0.5, 0.0, -0.5, 0.5])
            continue
        elif variant == "diffuse":
            gx, gy = _pt_lattice(11, 11, 0.05, "centre", 0.0)
        elif m == 476:
            gx, gy = _pt_lattice(21, 25, 0.05, "corner", 0.2)
        else:
            gx, gy = _pt_lattice(13, 13, 0.05, "corner", 0.2)
        assert gx.size == m
        for g in range(5):
            ox, oy = PT_OFFSETS[g]
            w = who[g * m:(g + 1) * m]
            lon[w] = cx + ox + gx; la[w] = cy + oy + gy
    lon[lab == 0] = -15.0; la[lab == 0] = 8.0
    lon[lab == 8] = 15.0; la[lab == 8] = -8.0
    live = np.arange(n) % 7 != 0
    x = np.asarray(sc["xtra1"]).copy(); y = np.asarray(sc["ytra1"]).copy()
    x[live] = lon + 20.0; y[live] = la + 12.0
    npoint = (1 + np.arange(n) % numpoint).astype(np.int32)
    npoint[live] = lab
    zs = np.array([50.0, 300.0, 900.0, 2500.0, 6000.0, 9000.0, 11500.0, 14000.0])
    z = zs[(_splitmix64(n, 0x971A) % np.uint64(8)).astype(np.int64)] * (0.75 + 0.5 * _uniform01(n, 0x971B))
    itra1 = np.where(live, 0, DEAD).astype(np.int32)
    sc.update(xtra1=x, ytra1=y, ztra1=z, npoint=npoint, itra1=itra1, itime=0)
    assert x[live].min() > 0.5 and x[live].max() < 38.5 and y[live].min() > 0.5 and y[live].max() < 22.5
    return sc


DF_VARIANTS = ("fill1", "fill2", "xglobal", "gdomainfill", "full")
DF_CALLS = 4
DF_NUMCOLUMN = (0, 1, 3, 4, 6)                       # never 2: boundcond_domainfill.f90:117 would read zcolumn(.., 0)
DF_MAXCOLUMN = 6


def domainfill_case(name="fill1"):
    """A scenario for boundcond_domainfill.f90 (mdomainfill = 1, 2), from integer hashes and IEEE-exact operations only, so
    that the tests regenerate the fixture's inputs bit for bit.  Met grid 12 x 10 x 8, one degree in y from -4.5: the filling
    box nx_we = (2, 9), ny_sn = (1, 8) straddles the equator (rows -3.5 .. 3.5 degrees).  memind = (2, 1); winds of both
    signs on every boundary; PV in pvu, signed like the latitude in most columns and against it in some, |PV| passing 2
    near 7 km.  The columns of release heights hold 0, 1, 3, 4 or 6 heights between 400 m and 16 km (numcolumn, zcolumn and
    acc_mass as [j][row][k], the host's (k, row, j) in memory order, compact: DF_MAXCOLUMN heights, nx | ny rows).  200
    storage spaces, about 150 live particles (itra1 = itime), vacancies in the middle (terminated, or born later), and live
    particles outside each of the four edges.  DF_CALLS calls at itime = 0, 900, ..: between two calls the caller moves
    itra1 of the live particles on by lsynctime, as the particle loop would (positions stay).
      fill1        mdomainfill = 1
      fill2        mdomainfill = 2: candidates rejected for z <= 3000, for pv <= pvcrit, and accepted
      xglobal      mdomainfill = 1, xglobal with nx_we = (0, nx-2): no termination in x
      gdomainfill  the routine returns at once
      full         mdomainfill = 1 with 10 vacancies only: the first call needs more"""
    if name not in DF_VARIANTS:
        raise ValueError(name)
    nx, ny, nz, cap = 12, 10, 8, 200
    xg = name == "xglobal"
    height = make_height(nz, top=30000.0, lin=0.15)
    f = make_fields(nx, ny, nz, height)
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[:, None, None]
    z = height[:, None, None]
    pv = np.empty((2, nz, ny, nx))
    for m in range(2):
        f["uu"][m] = 6.0 * _wave(3 * j + 2 * k + 5 * m + 0 * i, 13) + 2.0 * _wave(i + m, 7)
        f["vv"][m] = 5.0 * _wave(2 * i + 3 * k + 4 * m + 0 * j, 11) + 1.5 * _wave(j + 2 * m, 5)
        sign = np.where(2 * j - 9 > 0, 1.0, -1.0) * np.where((i + 2 * j) % 7 == 3, -1.0, 1.0)
        pv[m] = sign * (0.25 + z / 4000.0) * (1.0 + 0.25 * _wave(i + 3 * j + k + 2 * m, 9))
    sc = dict(
        grid=np.array([nx, ny, nz], np.int32),
        geom=np.array([360.0 / (nx - 1) if xg else 1.0, 1.0, -180.0 if xg else -6.0, -4.5], np.float64),
        globalflags=np.array([int(xg), 0, 0], np.int32), height=height, nmixz=nmixz_from_height(height),
        memtime=np.array([-1800, 9000], np.int32), memind=np.array([2, 1], np.int32),
        ldirect=1, lsynctime=900, method=1, mintime=225, ctl=5.0, ifine=4, turbswitch=1, cblflag=0,
        mdomainfill=2 if name == "fill2" else 1, lsettling=0, nspec=1, drydep=0, drydepspec=np.zeros(1, np.int32),
        density=np.zeros(1), dquer=np.zeros(1), vsetaver=np.zeros(1), cunningham=np.ones(1), decay=np.zeros(1),
        turbpar=np.array([50.0, 0.1, 0.16]), lage=np.array([999999999], np.int32), nsteps=1, itime0=0, itime=0,
        par_nxmax=361, npart=cap)
    sc.update(f)
    sc["pv"] = pv
    sc["qv"] = 0.0 * pv + 0.001
    sc["oro"] = np.zeros((ny, nx))
    sc["nx_we"] = np.array([0, nx - 2] if xg else [2, 9], np.int32)
    sc["ny_sn"] = np.array([1, 8], np.int32)
    sc["gdomainfill"] = int(name == "gdomainfill")
    sc["nclassunc"], sc["itsplit"], sc["ipout_df"] = 1, 7200, 1
    sc["xmassperparticle"] = 3.0e13 if xg else 2.5e12
    mc = DF_MAXCOLUMN
    for side, nrow in (("we", ny), ("sn", nx)):
        r = np.arange(nrow, dtype=np.int64)[:, None]
        kk = np.arange(2, dtype=np.int64)[None, :]
        ncol = np.array(DF_NUMCOLUMN, np.int64)[(2 * r + kk + (1 if side == "sn" else 0)) % 5]
        jj = np.arange(1, mc + 1, dtype=np.int64)[:, None, None]
        zc = 400.0 + (jj - 1) * np.floor(15600.0 / np.maximum(ncol[None], 1)) + 16.0 * ((3 * r[None] + 5 * kk[None] + 7 * jj) % 9)
        zc = np.where(jj <= ncol[None], zc, 0.0)
        h = _uniform01(mc * nrow * 2, 0xD0F1 + (side == "sn")).reshape(mc, nrow, 2)
        acc = np.where(jj <= ncol[None], np.floor(h * h * 3.6e12 / 1.0e6) * 1.0e6, 0.0)
        sc["numcolumn_" + side], sc["zcolumn_" + side], sc["acc_mass_" + side] = ncol.astype(np.int32), zc, acc
    # particles
    n = cap
    u1, u2, u3 = _uniform01(n, 0xD0F3), _uniform01(n, 0xD0F4), _uniform01(n, 0xD0F5)
    x0, x1 = float(sc["nx_we"][0]), float(sc["nx_we"][1])
    x = np.floor((x0 + 0.1 + (x1 - x0 - 0.2) * u1) * 1024.0) / 1024.0
    y = np.floor((1.1 + 6.8 * u2) * 1024.0) / 1024.0
    zt = np.floor(12000.0 * u3 * u3 * 64.0) / 64.0 + 10.0
    idx = np.arange(n)
    itra1 = np.zeros(n, np.int32)
    if name == "full":
        itra1[idx % 50 == 4] = DEAD                    # 4 vacancies, and 6 more by termination
    else:
        itra1[(idx % 5 == 2) & (idx > 40) & (idx < 170)] = DEAD
        itra1[(idx % 11 == 3)] = 900                   # born later: vacant at itime = 0, live at the second call
        itra1[190:] = DEAD
    out = {7: (x0 - 0.25, None), 23: (x1 + 0.5, None), 57: (None, 0.75), 88: (None, 8.125), 121: (x0 - 1.0, 8.5), 150: (x1 + 0.125, 4.0),
           13: (x0, 1.0), 14: (x1, 8.0)}              # the last two sit exactly on the edges: they stay
    for p, (px, py) in out.items():
        itra1[p] = 0
        if px is not None:
            x[p] = px
        if py is not None:
            y[p] = py
    h = _splitmix64(n, 0xD0F6)
    sc.update(xtra1=x, ytra1=y, ztra1=zt, itra1=itra1, itramem=np.where(itra1 == DEAD, 0, itra1).astype(np.int32),
              npoint=(idx + 1).astype(np.int32), nclass=np.ones(n, np.int32), idt=np.full(n, 225, np.int32),
              itrasplit=np.full(n, 7200, np.int32), xmass1=((1.0 + (h % np.uint64(64)).astype(np.float64)) * 1.0e10)[None, :],
              numpart=190 if name != "full" else 200, numparticlecount=n)
    return sc


OH_DIRECTIONS = (1, -1)
OH_PAD = (3, 2, 1)                                   # nxmax - nx, nymax - ny, nzmax - nz of the host's arrays
OH_HOT, OH_WARM = (8, 3, 2), (7, 4, 2)               # (OHx, OHy, OHz), 0-based: the cells of the two special particles


def oh_case(ldirect=1):
    """Inputs for the reference's gethourlyOH and ohreaction, from integer patterns, hashes and IEEE-exact operations only,
    so that the tests regenerate the fixture's inputs bit for bit.
    Mother grid 12 x 10 x 8, dx 15, dy 6 from (30, -30): longitudes 30 .. 195, so the wrap of ohreaction.f90:102-104 is taken
    east of 180.  One nest of 8 x 6 columns at half the spacing from (60, -12): mother x 2 .. 5.5, y 3 .. 5.5.  OH grid
    9 x 7 x 4: lonOH -180 .. 180 by 45, latOH -45 .. 45 by 15, altOH 500, 2000, 5000, 10000 m -- altOHtop 2750, 6500, 12500,
    12500: the last two are always equal in the reference (:114-117), so minloc never picks level nzOH.  bdate is 31 January
    2020 23:10 (ldirect = 1; 1 February 00:10 for ldirect = -1): the second hourly field lies in the other month, and the sun
    stands over 190 E: the OH columns at 45 E and 90 E are dark (OH exactly 0), those from 135 E eastwards are lit.
    jrate_average is <= 0 where the OH columns (135 E, -30 N) and (180 E, -15 N) look.  tt differs by at least 8 K between
    neighbouring cells in every direction and between the slots; OH_field by more than 4 %.
    837 storage spaces (three blocks of 256, one wave, five lanes): 60 dead with in-domain positions, 270 inside the nest;
    z below 9000 m (OH levels 1, 2) except two special particles at 11000 m (level 3): space 5 in the cell OH_HOT whose OH is
    3e4 times the pattern's (ohrate |ltsample| > 800: exp underflows to 0), space 6 in OH_WARM (300 or 175 times: the factor is near
    0.1) with a mass of 4 tiny in species 1, which oh_masses() sets per real kind.
    Species 1: ohnconst 2.0, ohdconst 1200; species 2: ohcconst -9.99 (never touched); species 3: ohnconst 1.5, ohdconst -300.
    calls: the sequence of the time manager -- gethourlyOH(0), ohreaction in the first hour, gethourlyOH at the hour (advance),
    again inside it (nothing), ohreaction with memind = (2, 1): n of ohreaction.f90:85-87 is 1 in the first and 2 in the second
    ohreaction, whatever memind says."""
    if ldirect not in OH_DIRECTIONS:
        raise ValueError(ldirect)
    nx, ny, nz, n = 12, 10, 8, 837
    nxo, nyo, nzo = 9, 7, 4
    ld = int(ldirect)
    c = dict(grid=np.array([nx, ny, nz], np.int32), pad=OH_PAD, geom=np.array([15.0, 6.0, 30.0, -30.0], np.float64),
             height=make_height(nz, top=30000.0, lin=0.15), nest=(8, 6), nestgeom=(7.5, 3.0, 60.0, -12.0),
             ohgrid=np.array([nxo, nyo, nzo], np.int32), ldirect=ld, nspec=3, npart=n,
             lonOH=-180.0 + 45.0 * np.arange(nxo), latOH=-45.0 + 15.0 * np.arange(nyo), altOH=np.array([500.0, 2000.0, 5000.0, 10000.0]),
             lonjr=-179.5 + np.arange(360.0), latjr=-89.5 + np.arange(180.0),
             bdate=GV_BDATE + 16.0 + (23.0 * 3600.0 + 600.0) / 86400.0 if ld == 1 else GV_BDATE + 17.0 + 600.0 / 86400.0,
             ohcconst=np.array([1.0e-13, -9.99, 1.0e-14]), ohdconst=np.array([1200.0, -9.99, -300.0]), ohnconst=np.array([2.0, -9.99, 1.5]))
    m, k, j, i = np.meshgrid(np.arange(12), np.arange(nzo), np.arange(nyo), np.arange(nxo), indexing="ij")
    f = 1.0e6 * (1.0 + ((i * 5 + j * 3 + k * 7 + m * 2) % 11).astype(np.float64) / 16.0)
    f[:, OH_HOT[2], OH_HOT[1], OH_HOT[0]] *= 3.0e4
    f[:, OH_WARM[2], OH_WARM[1], OH_WARM[0]] *= 300.0 if ld == 1 else 175.0     # ohrate |ltsample| = 2.3 in the first ohreaction
    c["OH_field"] = f                                               # [12][nzOH][nyOH][nxOH] = Fortran (ix,jy,kz,m)
    m, j, i = np.meshgrid(np.arange(12), np.arange(180), np.arange(360), indexing="ij")
    jr = 2.0e-5 * (1.0 + ((i + 2 * j + 5 * m) % 16).astype(np.float64) / 32.0)
    jr[:, 59, 314] = -1.0                                           # the picks of lonOH = 135 (a tie: the first, 134.5), latOH = -30 (-30.5)
    jr[:, 74, 359] = 0.0                                            # lonOH = 180 (179.5), latOH = -15 (-15.5)
    c["jrate_average"] = jr                                         # [12][180][360]
    m, k, j, i = np.meshgrid(np.arange(2), np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c["tt"] = 200.0 + 8.0 * ((i * 7 + j * 13 + k * 29 + m * 17) % 12).astype(np.float64)   # [2][nz][ny][nx]
    s = 7700 + (0 if ld == 1 else 50)
    u, v, w = _uniform01(n, s + 1), _uniform01(n, s + 2), _uniform01(n, s + 3)
    xt = 0.03 + 10.94 * u
    yt = 0.03 + 8.94 * v
    idx = np.arange(n)
    inn = idx % 3 == 1                                              # into the nest: x 2 .. 5.5, y 3 .. 5.5
    inn[-9:] = False
    xt[inn] = 2.02 + 3.46 * u[inn]
    yt[inn] = 3.02 + 2.46 * v[inn]
    zt = 50.0 + 8900.0 * w * w
    # the special particles: lon 180 = x 10, lat 0 = y 5 (OH_HOT); lon 135 = x 7, lat 15 = y 7.5 (OH_WARM)
    xt[5], yt[5], zt[5] = 9.9, 5.1, 11000.0
    xt[6], yt[6], zt[6] = 7.1, 7.4, 11000.0
    h = _splitmix64(n, s + 4)
    mass = np.empty((3, n), np.float64)
    mass[0] = (1.0 + (h % np.uint64(1000)).astype(np.float64)) / 3000.0
    mass[1] = (1.0 + ((h >> np.uint64(16)) % np.uint64(1000)).astype(np.float64)) / 7000.0
    mass[2] = (1.0 + ((h >> np.uint64(32)) % np.uint64(1000)).astype(np.float64)) * 1.0e9
    itra1 = np.zeros(n, np.int32)
    dead = np.nonzero((idx % 14 == 9) & (idx > 6))[0][:60]
    itra1[dead] = DEAD
    c.update(xtra1=xt, ytra1=yt, ztra1=zt, xmass1=mass, itra1=itra1, tiny_particle=6, hot_particle=5)
    c["calls"] = (("hourly", 0), ("react", 900 * ld, 900 * ld, (0, 10800 * ld), (1, 2)), ("hourly", 3600 * ld), ("hourly", 4500 * ld),
                  ("react", 6300 * ld, 900 * ld, (0, 10800 * ld), (2, 1)))
    return c


def oh_masses(c, kind):
    """xmass1 [3][n] of oh_case() in the real kind ('r4' | 'r8'), with the mass of 4 tiny(0.0) of that kind in place."""
    rt = np.float32 if kind == "r4" else np.float64
    m = np.asarray(c["xmass1"]).astype(rt)
    m[0, int(c["tiny_particle"])] = rt(4.0) * np.finfo(rt).tiny
    return m
