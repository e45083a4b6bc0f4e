"""TEST INFRASTRUCTURE ONLY -- the output-grid scatter of conccalc.f90, wetdepokernel(_nest).f90 and
drydepokernel(_nest).f90 restated in numpy, a builder of particle clouds laid out wave by wave, and exact sums.

The device code under test (flexpart_amd/csrc/fpx_device.hpp: wave_kernel_add, wave_total, wave_run_add and their
callers conccalc_particle, wetdepo_scatter, drydepo_particle) groups the 64 lanes of a wave by target cell before it
issues atomics.  Particle i of an upload sits in slot i, so a cloud built here decides which lanes share a cell.

Everything in the pattern cloud is dyadic: dx = dy = 1, dxout = 1/2, dxoutn = 1/4, masses small integers times 2**-10,
weight = 1/2, and positions in eighths of a cell of the grid a pattern is laid out on.  A pattern laid out on the mother
output grid has xl, yl in eighths there and in quarters on the nested grid; one laid out on the nested grid has them in
eighths there and in sixteenths on the mother grid.  All kernel weights are therefore multiples of 1/256 (1/64 on the
grid of the pattern), every contribution to gridunc is an integer multiple of QUANTUM = 2**-19 of at most a few thousand
quanta, and every partial sum is exact in float32 as well as in float64: the order of summation cannot matter and the
device has to reproduce the sums bit for bit.

The restatement is written from the Fortran in the given real kind R (np.float32 / np.float64), one numpy expression
per Fortran expression, and returns (flat index into the grid, value) per contribution; cells are summed with
math.fsum.  Three guards have no counterpart in the reference and are the engine's (a particle outside the met
domain or with a NaN height is not sampled, and neither is one whose class, point or age has no plane in the grids):
the restatement applies them, and `Cloud.oracle_view()` hands the C oracle -- which, like the Fortran, would index
out of bounds -- the same cloud with those lanes marked "not due".
"""
from __future__ import annotations

import math

import numpy as np

from flexpart_amd import synthetic as syn

ITIME = 7200
OLD, YOUNG, MIDDLE, ANCIENT = 20000, 3600, 30000, 50000      # age classes 2, 1, 2, none (lage = 10800, 43200)
DEAD = -999999999
NSPEC = 5
NXG, NYG, NZG = 16, 12, 3
NXN, NYN = 8, 8
OUT0 = (10.0, 8.0)           # origin of the mother output grid in met-grid coordinates (cells of 1/2)
NEST0 = (12.0, 10.0)         # origin of the nested output grid (cells of 1/4): mother cells 4..7 x 4..7
OUTHEIGHT = (100.0, 500.0, 1500.0)
ZLEV = (50.0, 300.0, 1000.0)     # a height inside each output level
LAGE = (10800, 43200)
NCLASSUNC, NUMPOINT = 3, 3
WEIGHT = 0.5
QUANTUM = 2.0 ** -19         # mass quantum 2**-10 x weight 2**-1 x kernel weight quantum 2**-8 (see the module docstring)
INACTIVE = ("notdue", "dead", "outside", "nanz", "above", "nclass0", "nclass4", "zeromass")
GUARDED = ("outside", "nanz", "nclass0", "nclass4")      # the engine's guards (see the module docstring)
RECEPTORS = ((12.5, 10.5), (25.0, 6.0), (6.0, 18.0), (30.0, 18.0))


def eps_of(R):
    """Unit roundoff of the real kind."""
    return 2.0 ** -24 if np.dtype(R) == np.float32 else 2.0 ** -53


# --------------------------------------------------------------------------------------------------------------
# scenario
# --------------------------------------------------------------------------------------------------------------
def scenario(cloud=None, *, lusekerneloutput=1, wet=None, nspec=NSPEC):
    """The base scenario of the scatter tests: 40 x 24 met grid of unit cells, a 16 x 12 x 3 output grid of half cells
    strictly inside it, an 8 x 8 nested output grid of quarter cells inside that, no density division, three release
    points, three uncertainty classes, two age classes, four receptors.  wet: None | "aerosol" | "gas"."""
    sc = syn.base_scenario(nx=40, ny=24, nz=30, global_grid=False, turb_off=True, nspec=nspec, nsteps=1)
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    assert (dx, dy, xlon0, ylat0) == (1.0, 1.0, -20.0, 20.0)
    sc["itime0"] = ITIME
    sc["outgrid"] = np.array([NXG, NYG, NZG], np.int32)
    sc["outgeom"] = np.array([0.5, 0.5, xlon0 + OUT0[0], ylat0 + OUT0[1]])
    sc["outheight"] = np.array(OUTHEIGHT)
    sc["concflags"] = np.array([0, 1], np.int32)             # ind_samp = 0, ioutputforeachrelease = 1
    sc["outtimes"] = np.array([10800, 3600], np.int32)
    sc["outgridn"] = np.array([NXN, NYN], np.int32)
    sc["outgeomn"] = np.array([0.25, 0.25, xlon0 + NEST0[0], ylat0 + NEST0[1]])
    sc["numpoint"] = NUMPOINT
    sc["xmass"] = np.ones((nspec, NUMPOINT))
    sc["npart_rel"] = np.full(NUMPOINT, 1000, np.int32)
    sc["nclassunc"] = NCLASSUNC
    sc["lage"] = np.array(LAGE, np.int32)
    sc["lusekerneloutput"] = int(lusekerneloutput)
    rx, ry = (np.array(v) for v in zip(*RECEPTORS))
    sc["receptors"] = np.concatenate([rx, ry, np.array([3.0e9, 5.0e9, 7.0e9, 9.0e9])])
    if wet is not None:
        syn.add_wet(sc, gas=(wet == "gas"))
        for k in ("weta_gas", "wetb_gas", "crain_aero", "csnow_aero", "ccn_aero", "in_aero", "henry"):
            sc[k] = np.full(nspec, float(np.asarray(sc[k])[0]))
        sc["wetdepspec"] = np.array([1, 0, 1, 1, 0][:nspec], np.int32)
        sc["dquer"] = np.full(nspec, 0.0 if wet == "gas" else 8.0)
    if cloud is not None:
        sc.update(cloud.arrays())
    return sc


# --------------------------------------------------------------------------------------------------------------
# cloud builder
# --------------------------------------------------------------------------------------------------------------
def _lane(xl, yl, grid="m", lev=0, age=OLD, kp=1, nc=1, kind="ok"):
    """One particle: (xl, yl) in cells of the mother ("m") or the nested ("n") output grid."""
    return dict(xl=float(xl), yl=float(yl), grid=grid, lev=lev, age=age, kp=kp, nc=nc, kind=kind)


def _off(l):
    """A position inside a cell in eighths, all four quadrants, the cell's middle lines and its lower edges included."""
    return ((3 * l) % 8) / 8.0, ((l // 8) * 3 + 5 * l + 2) % 8 / 8.0


_LO, _HI = (1 / 8, 2 / 8, 3 / 8), (5 / 8, 6 / 8, 7 / 8)


def _patterns():
    """name -> 64 lanes.  What each pattern makes wave_kernel_add do is tabulated in DESIGN.md."""
    A, B = (5, 5), (9, 3)
    w = {}

    def at(c, l, **kw):
        fx, fy = _off(l)
        return _lane(c[0] + fx, c[1] + fy, **kw)
    w["one_cell_one_quadrant"] = [_lane(A[0] + _HI[l % 3], A[1] + _HI[(l // 3) % 3]) for l in range(64)]
    w["one_cell_four_quadrants"] = [at(A, l) for l in range(64)]
    w["two_cells_alternating"] = [at(A if l % 2 == 0 else B, l) for l in range(64)]
    small = {10: (8, 8), 20: (2, 9), 41: (2, 9), 5: (11, 2), 30: (11, 2), 55: (11, 2)}
    w["groups_1_2_3_big_first"] = [at(small.get(l, A), l) for l in range(64)]
    small = {0: (8, 8), 1: (2, 9), 2: (2, 9), 3: (11, 2), 4: (11, 2), 5: (11, 2)}
    w["groups_1_2_3_small_first"] = [at(small.get(l, A), l) for l in range(64)]
    cells8 = [(4, 4), (5, 4), (6, 4), (7, 4), (4, 6), (5, 6), (6, 6), (10, 9)]
    w["eight_cells_of_eight"] = [at(cells8[l % 8], l) for l in range(64)]
    w["distinct_64"] = [at((l % 16, 2 + l // 16), l) for l in range(64)]
    w["same_cell_three_levels"] = [at(A, l, lev=l % 3) for l in range(64)]
    w["same_cell_three_classes"] = [at(A, l, nc=1 + l % 3) for l in range(64)]
    w["same_cell_three_points"] = [at(A, l, kp=1 + l % 3) for l in range(64)]
    w["same_cell_ages"] = [at(A, l, age=(OLD, YOUNG, MIDDLE, ANCIENT)[l % 4]) for l in range(64)]
    w["inactive_even_lanes"] = [at(A, l, kind=INACTIVE[(l // 2) % 8]) if l % 2 == 0 else at(A, l) for l in range(64)]
    w["inactive_odd_lanes"] = [at(A, l, kind=INACTIVE[(l // 2) % 8]) if l % 2 == 1 else at(A, l) for l in range(64)]
    w["no_active_lane"] = [at(A, l, kind="notdue") for l in range(64)]

    def edge(l, n):   # along one axis of n cells: first cell / last cell / one cell outside on either side
        k = l // 4
        return (_LO[k % 3], n - 1 + _HI[k % 3], -_LO[k % 3], n + _LO[k % 3])[l % 4]
    w["edges_x"] = [_lane(edge(l, NXG), 5 + _off(l)[1]) for l in range(64)]
    w["edges_y"] = [_lane(6 + _off(l)[0], edge(l, NYG)) for l in range(64)]
    w["corners"] = [_lane(edge(2 * (l % 2) + (l // 8) % 2 + 4 * (l // 16), NXG), edge(2 * ((l // 2) % 2) + (l // 8) % 2 + 4 * (l // 16), NYG))
                    for l in range(64)]
    ring = [(-1.25, 5.5), (NXG + 1.25, 5.5), (5.5, -1.25), (5.5, NYG + 1.25)]
    w["two_cells_outside"] = [at(A, l) if l < 3 else _lane(*ring[l % 4]) for l in range(64)]
    # nested grid, floor(): (ix = -1, jy = 4) and (ix = 7, jy = 3) have the same linear index, (8, 3) and (0, 4) too
    alias = [(-0.25, 4.0), (7.0, 3.0), (8.25, 3.0), (0.0, 4.0)]
    w["alias_pairs_nest"] = [_lane(alias[l % 4][0] + (l // 4 % 2) * (0.5 if l % 4 in (1, 3) else 0.0), alias[l % 4][1] + _off(l)[1], grid="n")
                             for l in range(64)]
    # the first plane (species 1, point 1, class 1, age class 1) with jy = -1: a negative linear index
    w["negative_index_nest"] = [_lane(3 + _off(l)[0] if l % 2 == 0 else -0.25, -0.25, grid="n", age=YOUNG) for l in range(64)]
    w["direct_young"] = [at(A, l, age=YOUNG) for l in range(64)]
    lo, hi = (0.0, 1 / 8, 3 / 8, 0.5), (0.5, 5 / 8, 7 / 8, 1.0 - 1 / 8)
    w["direct_low_edge"] = [_lane(lo[l % 4], 5 + _off(l)[1]) if l < 32 else _lane(5 + _off(l)[0], lo[l % 4]) for l in range(64)]
    w["direct_high_edge"] = [_lane(NXG - 2 + hi[l % 4], 5 + _off(l)[1]) if l < 32 else _lane(5 + _off(l)[0], NYG - 2 + hi[l % 4])
                             for l in range(64)]
    w["nest_inside"] = [at((1 + l % 6, 1 + (l // 6) % 6), l, grid="n") for l in range(64)]
    w["nest_border"] = [_lane((lo[l % 4], NXN - 2 + hi[l % 4])[(l // 4) % 2], 1 + (l % 6) + _off(l)[1], grid="n") if l < 32 else
                        _lane(1 + (l % 6) + _off(l)[0], (lo[l % 4], NYN - 2 + hi[l % 4])[(l // 4) % 2], grid="n") for l in range(64)]
    w["nest_outside"] = [_lane(edge(l, NXN), 3 + _off(l)[1], grid="n") if l < 32 else _lane(3 + _off(l)[0], edge(l, NYN), grid="n")
                         for l in range(64)]
    assert all(len(v) == 64 for v in w.values())
    return w


class Cloud:
    """Scenario arrays of a cloud plus pattern -> slot range."""

    def __init__(self, lanes, ranges, *, wet=False):
        n = len(lanes)
        self.n, self.ranges, self.kinds = n, ranges, [L["kind"] for L in lanes]
        x = np.empty(n); y = np.empty(n); z = np.empty(n)
        itra1 = np.full(n, ITIME, np.int32); itramem = np.empty(n, np.int32)
        npoint = np.empty(n, np.int32); nclass = np.empty(n, np.int32)
        k = 1 + (np.arange(n) * 7) % 5
        mass = (k[None, :] + 2 * np.arange(NSPEC)[:, None]) * 2.0 ** -10       # differs per species, small integers x 2**-10
        self.guarded = np.zeros(n, bool)
        for i, L in enumerate(lanes):
            o, cell = (OUT0, 0.5) if L["grid"] == "m" else (NEST0, 0.25)
            x[i], y[i] = o[0] + L["xl"] * cell, o[1] + L["yl"] * cell
            # wet clouds: below the precipitating cloud (clouds = 6 under 1200 m) and inside it (3 under 5000 m)
            z[i] = ((400.0, 2500.0, 800.0)[i % 3] if wet else ZLEV[L["lev"]])
            itramem[i] = ITIME - L["age"]
            npoint[i], nclass[i] = L["kp"], L["nc"]
            kind = L["kind"]
            if kind == "notdue": itra1[i] = ITIME + 900
            elif kind == "dead": itra1[i] = DEAD
            elif kind == "outside": x[i], y[i] = ((-0.5, y[i]), (39.5, y[i]), (x[i], -0.25), (x[i], 23.5))[i % 4]
            elif kind == "nanz": z[i] = np.nan
            elif kind == "above": z[i] = 2000.0
            elif kind == "nclass0": nclass[i] = 0
            elif kind == "nclass4": nclass[i] = NCLASSUNC + 1
            elif kind == "zeromass": mass[:, i] = 0.0
            else: assert kind == "ok", kind
            self.guarded[i] = kind in GUARDED
        self.a = dict(npart=n, xtra1=x, ytra1=y, ztra1=z, itra1=itra1, itramem=itramem, npoint=npoint, nclass=nclass, xmass1=mass)

    def arrays(self, n=None):
        n = self.n if n is None else n
        return {k: (n if k == "npart" else (v[:, :n] if k == "xmass1" else v[:n]).copy()) for k, v in self.a.items()}

    def oracle_view(self, n=None):
        """The same cloud for the C oracle: the lanes only the engine guards are marked not due (it would index out of bounds)."""
        a = self.arrays(n)
        a["itra1"][self.guarded[: a["npart"]]] = ITIME + 900
        a["ztra1"] = np.where(np.isnan(a["ztra1"]), 50.0, a["ztra1"])
        a["nclass"] = np.clip(a["nclass"], 1, NCLASSUNC)
        return a


def pattern_cloud(*, wet=False):
    """Every pattern, one wave each, then one more particle: 64 k + 1 slots (a partial last wave)."""
    lanes, ranges = [], {}
    for name, wave in _patterns().items():
        ranges[name] = (len(lanes), len(lanes) + 64)
        lanes += wave
    ranges["tail"] = (len(lanes), len(lanes) + 1)
    lanes.append(_lane(5.75, 5.25))
    assert len(lanes) % 64 == 1 and len(lanes) <= 30 * 64
    return Cloud(lanes, ranges, wet=wet)


def receptor_cloud():
    """Hit / miss lane patterns of the receptor kernel, one wave each; wave k belongs to receptor k % 4.  A hit sits within
    half a kernel width of its receptor in every direction, a miss three cells to the east (xd**2 > 10)."""
    pats = {
        "all_hit": [True] * 64,
        "alternating": [l % 2 == 0 for l in range(64)],
        "exactly_two": [l in (17, 40) for l in range(64)],
        "exactly_three": [l in (3, 31, 32) for l in range(64)],
        "lanes_0_and_63": [l in (0, 63) for l in range(64)],
        "run_with_a_gap": [10 <= l <= 40 and l != 25 for l in range(64)],
    }
    lanes, ranges, rec = [], {}, []
    for k, (name, hits) in enumerate(pats.items()):
        ranges[name] = (len(lanes), len(lanes) + 64)
        rx, ry = RECEPTORS[k % 4]
        for l, hit in enumerate(hits):
            ddx, ddy = ((l % 7) - 3) / 8.0, ((l % 5) - 2) / 16.0        # |ddx| <= 0.375 < hx / 2, |ddy| <= 0.125 < hy / 2
            lanes.append(dict(x=rx + ddx + (0.0 if hit else 3.0), y=ry + ddy, z=5.0 + (l % 9) * 4.0, hit=hit))
            rec.append(k % 4)
    n = len(lanes)
    c = Cloud([_lane(5.5, 5.5)] * n, ranges)
    c.a["xtra1"] = np.array([L["x"] for L in lanes]); c.a["ytra1"] = np.array([L["y"] for L in lanes])
    c.a["ztra1"] = np.array([L["z"] for L in lanes])
    c.a["xmass1"] = (1.0 + 0.37 * np.arange(NSPEC)[:, None]) * (0.6 + 0.013 * (np.arange(n) % 29))[None, :]   # not dyadic
    c.want_hit, c.receptor_of = np.array([L["hit"] for L in lanes]), np.array(rec)
    return c


# --------------------------------------------------------------------------------------------------------------
# restatement
# --------------------------------------------------------------------------------------------------------------
def _geom(sc, R, nest):
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    dxo, dyo, lon0, lat0 = (float(v) for v in sc["outgeomn" if nest else "outgeom"])
    numx, numy = (int(v) for v in (sc["outgridn"] if nest else sc["outgrid"][:2]))
    # xoutshift = xlon0 - outlon0 in the default real kind, readoutgrid.f90:199-200
    return dict(dx=R(dx), dy=R(dy), dxout=R(dxo), dyout=R(dyo), xshift=R(R(xlon0) - R(lon0)), yshift=R(R(ylat0) - R(lat0)),
                numx=numx, numy=numy)


def _planes(sc, p, itime):
    """(itage, nage, kp, planes_ok): age class conccalc.f90:54-58, release point :130-134; planes_ok is the engine's guard."""
    lage = np.asarray(sc["lage"]).ravel()
    itage = np.abs(itime - p["itramem"].astype(np.int64))
    nage = 1 + np.searchsorted(lage, itage, side="right")
    iofr = int(np.asarray(sc["concflags"]).ravel()[1])
    mps = int(sc.get("numpoint", 1)) if iofr == 1 else 1
    ncu = int(sc.get("nclassunc", 1))
    kp = p["npoint"].astype(np.int64) if iofr == 1 else np.ones(len(itage), np.int64)
    nc = p["nclass"].astype(np.int64)
    ok = (nage <= len(lage)) & (nc >= 1) & (nc <= ncu) & (kp >= 1) & (kp <= mps)
    return itage, nage, kp, nc, ok, (len(lage), ncu, mps)


def _in_domain(sc, p):
    nx, ny = int(sc["grid"][0]), int(sc["grid"][1])
    x, y, z = p["xtra1"], p["ytra1"], p["ztra1"]
    return (x >= 0) & (x <= nx - 1) & (y >= 0) & (y <= ny - 1) & (z == z)


def _kernel(xl, yl, ix, jy, R):
    """The uniform kernel, conccalc.f90:196-213 = wetdepokernel.f90:60-77 = drydepokernel.f90:68-85:
    -> four (ix, jy, weight) targets in the order the Fortran adds them to the own cell, (ixp, jyp), (ixp, jy), (ix, jyp)."""
    ddx, ddy = xl - ix.astype(R), yl - jy.astype(R)
    hx, hy = ddx > R(0.5), ddy > R(0.5)
    ixp, wx = np.where(hx, ix + 1, ix - 1), np.where(hx, R(1.5) - ddx, R(0.5) + ddx)
    jyp, wy = np.where(hy, jy + 1, jy - 1), np.where(hy, R(1.5) - ddy, R(0.5) + ddy)
    one = R(1.0)
    out = [(ix, jy, wx * wy), (ixp, jyp, (one - wx) * (one - wy)), (ixp, jy, (one - wx) * wy), (ix, jyp, wx * (one - wy))]
    assert all(t[2].dtype == np.dtype(R) for t in out)
    return out


def conccalc_contribs(sc, p, R, *, itime=ITIME, weight=WEIGHT, nest=False):
    """conccalc.f90:140-295 (mother grid) / :301-441 (nested grid), ind_samp = 0: -> (idx, val) of every addition to
    gridunc / griduncn, idx into the C-ordered (age, class, point, species, z, y, x) array, val in the real kind R."""
    R = np.dtype(R).type
    G = _geom(sc, R, nest)
    nspec = int(sc["nspec"])
    assert int(np.asarray(sc["concflags"]).ravel()[0]) == 0, "the restatement has no density division"
    itage, nage, kp, nc, planes_ok, (_, ncu, mps) = _planes(sc, p, itime)
    z = p["ztra1"].astype(R)
    oh = np.asarray(sc["outheight"]).astype(R)
    kz = 1 + np.searchsorted(oh, np.where(z == z, z, R(0)), side="right")       # first level with outheight > z
    active = (p["itra1"] == itime) & _in_domain(sc, p) & planes_ok & (kz <= len(oh))
    xl = ((p["xtra1"] * float(G["dx"]) + float(G["xshift"])) / float(G["dxout"])).astype(R)
    yl = ((p["ytra1"] * float(G["dy"]) + float(G["yshift"])) / float(G["dyout"])).astype(R)
    ix = xl.astype(np.int64) - (xl < 0)
    jy = yl.astype(np.int64) - (yl < 0)
    numx, numy = G["numx"], G["numy"]
    direct = (not int(sc.get("lusekerneloutput", 1))) | (itage < 10800) | (xl < R(0.5)) | (yl < R(0.5)) | \
        (xl > R(numx - 1) - R(0.5)) | (yl > R(numy - 1) - R(0.5))
    lead = ((nage - 1) * ncu + (nc - 1)) * mps + (kp - 1)
    targets = [(ix, jy, None, active & direct)] + [(i, j, w, active & ~direct) for i, j, w in _kernel(xl, yl, ix, jy, R)]
    xm = np.asarray(p["xmass1"]).astype(R).reshape(nspec, -1)
    idx, val = [], []
    for ks in range(nspec):
        m = xm[ks] / R(1.0) * R(weight)
        for i, j, w, on in targets:
            on = on & (i >= 0) & (i <= numx - 1) & (j >= 0) & (j <= numy - 1)
            v = m if w is None else m * w
            idx.append(((((lead * nspec + ks) * len(oh) + (kz - 1)) * numy + j) * numx + i)[on])
            val.append(v[on])
    val = np.concatenate(val)
    assert val.dtype == np.dtype(R)
    return np.concatenate(idx), val


def depo_contribs(sc, x, y, R, deposit, species, nage, kp, nc, *, nest=False, kind="wet"):
    """wetdepokernel.f90 / wetdepokernel_nest.f90 / drydepokernel.f90 / drydepokernel_nest.f90 for particles at (x, y) (met
    grid coordinates, float64) with deposits `deposit` [nspec][n] (float64; 0 = none): -> dict of arrays with one entry per
    addition: idx into the C-ordered (age, class, point, species, y, x) array, val = float32(R(deposit) * w) as the dep_prec
    grid receives it, w the kernel weight, particle and species of the addition.  Planes outside the grids are left out (the engine's guard)."""
    R = np.dtype(R).type
    G = _geom(sc, R, nest)
    nspec = int(sc["nspec"])
    xr, yr = np.asarray(x).astype(R), np.asarray(y).astype(R)
    xl = (xr * G["dx"] + G["xshift"]) / G["dxout"]
    yl = (yr * G["dy"] + G["yshift"]) / G["dyout"]
    assert xl.dtype == np.dtype(R)
    if kind == "wet" and nest:      # wetdepokernel_nest.f90 truncates with floor(), the other three with int()
        ix, jy = np.floor(xl).astype(np.int64), np.floor(yl).astype(np.int64)
    else:
        ix, jy = xl.astype(np.int64), yl.astype(np.int64)
    numx, numy = G["numx"], G["numy"]
    lage = np.asarray(sc["lage"]).ravel()
    iofr = int(np.asarray(sc["concflags"]).ravel()[1])
    mps = int(sc.get("numpoint", 1)) if iofr == 1 else 1
    ncu = int(sc.get("nclassunc", 1))
    ok = (nage >= 1) & (nage <= len(lage)) & (nc >= 1) & (nc <= ncu) & (kp >= 1) & (kp <= mps)
    lead = ((nage - 1) * ncu + (nc - 1)) * mps + (kp - 1)
    kern = nest or bool(int(sc.get("lusekerneloutput", 1)))         # the nested variants always use the kernel
    targets = _kernel(xl, yl, ix, jy, R) if kern else [(ix, jy, np.ones(len(xl), R))]
    idx, val, raw, wgt, own, spc = [], [], [], [], [], []
    for ks in species:
        d = np.asarray(deposit[ks]).astype(R)
        for i, j, w in targets:
            on = ok & (d != 0) & (i >= 0) & (i <= numx - 1) & (j >= 0) & (j <= numy - 1)
            idx.append((((lead * nspec + ks) * numy + j) * numx + i)[on])
            raw.append((d * w)[on] if kern else d[on])
            val.append(raw[-1].astype(np.float32))
            wgt.append(w.astype(np.float64)[on])
            own.append(np.flatnonzero(on))
            spc.append(np.full(int(on.sum()), ks))
    return dict(idx=np.concatenate(idx), val=np.concatenate(val), raw=np.concatenate(raw), w=np.concatenate(wgt),
                particle=np.concatenate(own), species=np.concatenate(spc))


def sum_cells(idx, val, size):
    """Exact sum (math.fsum, rounded once to float64) of the contributions of every cell -> float64 [size]."""
    out = np.zeros(size)
    if len(idx) == 0:
        return out
    order = np.argsort(idx, kind="stable")
    i, v = np.asarray(idx)[order], np.asarray(val, np.float64)[order]
    cells, start = np.unique(i, return_index=True)
    stop = list(start[1:]) + [len(i)]
    for c, a, b in zip(cells, start, stop):
        out[c] = math.fsum(v[a:b])
    return out


def count_cells(idx, size):
    return np.bincount(np.asarray(idx, np.int64), minlength=size).astype(np.float64)


def grid_size(sc, nest=False, levels=True):
    nxy = int(np.prod(sc["outgridn"])) if nest else int(sc["outgrid"][0]) * int(sc["outgrid"][1])
    iofr = int(np.asarray(sc["concflags"]).ravel()[1])
    mps = int(sc.get("numpoint", 1)) if iofr == 1 else 1
    return len(np.asarray(sc["lage"]).ravel()) * int(sc.get("nclassunc", 1)) * mps * int(sc["nspec"]) * \
        (int(sc["outgrid"][2]) if levels else 1) * nxy


def exact_gridunc(sc, p, R, *, nest=False, weight=WEIGHT, itime=ITIME):
    idx, val = conccalc_contribs(sc, p, R, itime=itime, weight=weight, nest=nest)
    return sum_cells(idx, val, grid_size(sc, nest))


# --------------------------------------------------------------------------------------------------------------
# receptor kernel, conccalc.f90:451-498
# --------------------------------------------------------------------------------------------------------------
def receptor_terms(sc, p, R, *, itime=ITIME, weight=WEIGHT):
    """-> dict(c [nspec][nrec][n]: every particle's share 2 weight xmass xkern / h / area in R (0 for a miss),
    hit [nrec][n], margin [nrec][n]: the least distance of zd, xd**2, yd**2, r2 from their threshold 1,
    part [nspec][nrec][n]: xmass xkern / h, the term the Fortran sums serially)."""
    R = np.dtype(R).type
    nspec = int(sc["nspec"])
    rec = np.asarray(sc["receptors"], np.float64).reshape(3, -1).astype(R)
    dx, dy = R(float(sc["geom"][0])), R(float(sc["geom"][1]))
    due = (p["itra1"] == itime) & _in_domain(sc, p)
    itage = np.abs(itime - p["itramem"].astype(np.int64)).astype(R)
    sq = np.sqrt(itage)
    z = p["ztra1"].astype(R)
    hz = np.minimum(R(50.) + R(0.3) * sq, R(150.))
    zd = z / hz
    hx = np.minimum((R(0.29) + R(2.222e-3) * sq) * dx + itage * R(1.2e-5), R(6.0))
    hy = np.minimum((R(0.18) + R(1.389e-3) * sq) * dy + itage * R(7.5e-6), R(4.0))
    h = hx * hy * hz
    xm = np.asarray(p["xmass1"]).astype(R).reshape(nspec, -1)
    nrec, n = rec.shape[1], len(z)
    c = np.zeros((nspec, nrec, n), R); part = np.zeros((nspec, nrec, n), R)
    hit = np.zeros((nrec, n), bool); margin = np.zeros((nrec, n))
    for r in range(nrec):
        xd = ((p["xtra1"] - float(rec[0, r])) / hx.astype(np.float64)).astype(R)
        yd = ((p["ytra1"] - float(rec[1, r])) / hy.astype(np.float64)).astype(R)
        r2 = xd * xd + yd * yd + zd * zd
        hit[r] = due & ~(zd > R(1.)) & ~(xd * xd > R(1.)) & ~(yd * yd > R(1.)) & (r2 < R(1.))
        margin[r] = np.min(np.abs(np.stack([zd, xd * xd, yd * yd, r2]).astype(np.float64) - 1.0), axis=0)
        xkern = R(.596831) * (R(1.) - r2)
        for ks in range(nspec):
            part[ks, r] = np.where(hit[r], xm[ks] * xkern / h, R(0))
            c[ks, r] = np.where(hit[r], R(2.) * R(weight) * (xm[ks] * xkern / h) / rec[2, r], R(0))
    assert c.dtype == np.dtype(R)
    return dict(c=c, hit=hit, margin=margin, part=part, area=rec[2])


def receptor_serial(sc, p, R, *, itime=ITIME, weight=WEIGHT):
    """creceptor [nspec][nrec] as the Fortran leaves it: the particles of a receptor summed one after the other in R, then
    2 weight sum / area."""
    R = np.dtype(R).type
    t = receptor_terms(sc, p, R, itime=itime, weight=weight)
    nspec, nrec, _ = t["part"].shape
    out = np.zeros((nspec, nrec), R)
    for ks in range(nspec):
        for r in range(nrec):
            v = t["part"][ks, r][t["hit"][r]]
            cc = np.cumsum(v, dtype=R)[-1] if len(v) else R(0)        # cumsum adds strictly left to right
            out[ks, r] = R(2.) * R(weight) * cc / t["area"][r]
    return out.astype(np.float64)


# --------------------------------------------------------------------------------------------------------------
# wet deposit of a particle when the scavenging saturates, and the serial accumulation of the reference
# --------------------------------------------------------------------------------------------------------------
SATURATING_LTSAMPLE = 2 ** 30


def wet_deposit_saturated(sc, p, R, *, itime=ITIME, ltsample=SATURATING_LTSAMPLE):
    """wetdepo.f90:58-151 with get_wetscav.f90:78-314 and interpol_rain.f90:68-130 (mother met grid, no nests, no decay) for a
    sampling time so long that 1 - exp(-wetscav |ltsample|) rounds to one wherever a particle is scavenged at all
    (wetscav > 4e-8 / s is enough in both real kinds; the scenarios' coefficients are far above).  The deposit is then
    xmass * grfraction, which needs the bilinear interpolation of the precipitation and the cloud class only -- no
    transcendental function, so it can be restated bit for bit.  -> (deposit [nspec][n], xmass1 afterwards [nspec][n]) in R."""
    R = np.dtype(R).type
    nspec = int(sc["nspec"])
    nx, ny = int(sc["grid"][0]), int(sc["grid"][1])
    dq = np.asarray(sc["dquer"]).ravel()
    for ks in range(nspec):      # the species are such that every cloudy, raining column scavenges (get_wetscav.f90:206-311)
        if dq[ks] > 0:
            assert sc["crain_aero"][ks] > 0 and sc["csnow_aero"][ks] > 0 and sc["ccn_aero"][ks] > 0
        else:
            assert sc["weta_gas"][ks] > 0 and sc["henry"][ks] > 0
    assert not np.any(np.asarray(sc["decay"]) > 0) and "nest" not in sc
    live = (p["itra1"] != DEAD) & (p["itra1"] <= itime)           # ldirect = 1
    x = np.where(live, p["xtra1"], 0.0); y = np.where(live, p["ytra1"], 0.0)
    z = np.where(live & (p["ztra1"] == p["ztra1"]), p["ztra1"], 0.0).astype(R)
    assert x.max() < nx - 1 and y.max() < ny - 1 and x.min() >= 0 and y.min() >= 0
    interp_time = int(np.round(np.float64(R(itime) - R(0.5) * R(ltsample))))
    mt, mi = np.asarray(sc["memtime"]), np.asarray(sc["memind"])
    m = int(mi[0] if abs(int(mt[0]) - interp_time) < abs(int(mt[1]) - interp_time) else mi[1]) - 1
    xt, yt = x.astype(R), y.astype(R)
    ix, jy = xt.astype(np.int64), yt.astype(np.int64)
    ddx, ddy = xt - ix.astype(R), yt - jy.astype(R)
    rddx, rddy = R(1.) - ddx, R(1.) - ddy
    p1, p2, p3, p4 = rddx * rddy, ddx * rddy, rddx * ddy, ddx * ddy

    def interp(key):
        f = np.asarray(sc[key]).astype(R)[m]
        return p1 * f[jy, ix] + p2 * f[jy, ix + 1] + p3 * f[jy + 1, ix] + p4 * f[jy + 1, ix + 1]
    lsp, convp, cc = interp("lsprec"), interp("convprec"), interp("tcc")
    hgt = np.asarray(sc["height"]).astype(R)
    k = np.searchsorted(hgt, z, side="right")                      # first level above the particle (0-based)
    hz = np.where(k < len(hgt), np.maximum(k, 1), 1)               # get_wetscav.f90:138-143
    clouds_v = np.asarray(sc["clouds"])[m][hz - 1, y.astype(np.int64), x.astype(np.int64)]
    wet = live & ~((lsp < R(0.01)) & (convp < R(0.01))) & (clouds_v > 1)
    lfr = np.array([0.5, 0.65, 0.8, 0.9, 0.95]).astype(R)
    cfr = np.array([0.4, 0.55, 0.7, 0.8, 0.9]).astype(R)
    cls = lambda v: (v > R(1.)).astype(int) + (v > R(3.)) + (v > R(8.)) + (v > R(20.))   # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        grfr = np.maximum(R(0.05), cc * (lsp * lfr[cls(lsp)] + convp * cfr[cls(convp)]) / (lsp + convp))
    assert grfr.dtype == np.dtype(R)
    xm = np.asarray(p["xmass1"]).astype(R).reshape(nspec, -1)
    tiny = np.finfo(R).tiny
    dep, after = np.zeros_like(xm), xm.copy()
    for ks in range(nspec):
        if not int(np.asarray(sc["wetdepspec"]).ravel()[ks]):
            continue
        dep[ks] = np.where(wet, xm[ks] * R(1.) * grfr, R(0))
        rest = xm[ks] - dep[ks]
        after[ks] = np.where(live, np.where(rest > tiny, rest, R(0)), xm[ks])
    return dep, after


def serial_depo_grid(sc, x, y, R, deposit, species, nage, kp, nc, *, nest, kind="wet"):
    """The dep_prec grid as the serial reference leaves it: grid = real(grid, dep_prec) of (real(grid) + deposit * w),
    particle after particle (a cell receives at most one addition per particle and species)."""
    R = np.dtype(R).type
    t = depo_contribs(sc, x, y, R, deposit, species, nage, kp, nc, nest=nest, kind=kind)
    order = np.lexsort((t["particle"], t["idx"]))
    out = np.zeros(grid_size(sc, nest, levels=False), np.float32)
    for c, v in zip(t["idx"][order], t["raw"][order]):
        out[c] = np.float32(R(out[c]) + v)
    return out.astype(np.float64)
