"""numpy restatement of partpos_average.f90:31-184 and partoutput_average.f90:54-201 in the reference's real kinds.

Every operation is one numpy ufunc on arrays of the host's real kind (float32 for 'r4', float64 for 'r8'), in the
reference's order, so nothing is contracted; where the reference mixes a double position with default reals the
expression is formed in float64 and rounded, as the Fortran assignment does.  Twelve of the fifteen arrays are therefore
the reference's bit for bit; the three Cartesian sums (and the two angles the writer derives from them) go through sin,
cos and atan2, which differ between libraries in the last bits (tests/test_partavg.py states the bound once).
"""
import numpy as np

RT = {"r4": np.float32, "r8": np.float64}
SUMS = ("cartx", "carty", "cartz", "z", "topo", "pv", "qv", "tt", "uu", "vv", "rho", "tro", "hmix", "energy")
EXACT = SUMS[3:]
DEAD = -999999999


class Params:
    """The fields and constants partpos_average reads, in the real kind `kind`.  Fields are compact arrays indexed by the
    physical time slot: [2][nz][ny][nx] and [2][ny][nx]; memind (1-based) names the slot of the window's two ends."""

    def __init__(self, src, kind, nymax=None):
        rt = self.rt = RT[kind]
        self.kind = kind
        self.nx, self.ny, self.nz = (int(v) for v in src["grid"])
        self.nymax = int(nymax if nymax is not None else src.get("nymax", self.ny))
        self.dx, self.dy, self.xlon0, self.ylat0 = (rt(v) for v in src["geom"])
        self.height = np.asarray(src["height"]).astype(rt)
        self.memtime = [int(v) for v in src["memtime"]]
        self.slot = [int(v) - 1 for v in np.asarray(src["memind"])[:2]]
        for k in ("oro", "pv", "qv", "tt", "uu", "vv", "rho", "tropopause", "hmix"):
            setattr(self, k, np.asarray(src[k]).astype(rt))
        self.pi180 = rt(3.14159265) / rt(180.)          # par_mod.f90:61-63
        self.cpa = rt(1004.6)


def new_state(n, kind):
    st = {k: np.zeros(n, RT[kind]) for k in SUMS}
    st["npart_av"] = np.zeros(n, np.int32)
    return st


def addends(P, itime, xt, yt, zt, stats=None):
    """partpos_average.f90:31-169 for the particles at (xt, yt, zt): the fourteen values one call adds, in SUMS order."""
    rt = P.rt
    xt = np.asarray(xt, np.float64); yt = np.asarray(yt, np.float64)
    zt = np.asarray(zt).astype(rt)
    dt1 = rt(itime - P.memtime[0]); dt2 = rt(P.memtime[1] - itime)
    dtt = rt(1.) / (dt1 + dt2)
    xlon = (np.float64(P.xlon0) + xt * np.float64(P.dx)).astype(rt)
    ylat = (np.float64(P.ylat0) + yt * np.float64(P.dy)).astype(rt)
    ix = xt.astype(np.int64); jy = yt.astype(np.int64)
    ixp = ix + 1; jyp = jy + 1
    ddx = (xt - ix.astype(rt).astype(np.float64)).astype(rt)
    ddy = (yt - jy.astype(rt).astype(np.float64)).astype(rt)
    rddx = rt(1.) - ddx; rddy = rt(1.) - ddy
    p1 = rddx * rddy; p2 = ddx * rddy; p3 = rddx * ddy; p4 = ddx * ddy
    fix = jyp >= P.nymax
    if stats is not None:
        stats["fixup"] = stats.get("fixup", 0) + int(fix.sum())
    jyp = np.where(fix, jyp - 1, jyp)
    assert ix.min() >= 0 and ixp.max() <= P.nx - 1 and jy.min() >= 0 and jyp.max() <= P.ny - 1, "position outside the grid"

    def h2(f):
        return p1 * f[jy, ix] + p2 * f[jy, ixp] + p3 * f[jyp, ix] + p4 * f[jyp, ixp]

    topo = h2(P.oro)
    above = P.height[None, 1:] > zt[:, None]             # first il in 2..nz with height(il) > ztra1
    indzp = np.where(above.any(axis=1), above.argmax(axis=1) + 1, P.nz - 1)      # 0-based index of height(indzp)
    indz = indzp - 1
    dz1 = zt - P.height[indz]; dz2 = P.height[indzp] - zt
    dz = rt(1.) / (dz1 + dz2)

    def prof(f):
        out = []
        for ind in (indz, indzp):
            v = [p1 * f[h][ind, jy, ix] + p2 * f[h][ind, jy, ixp] + p3 * f[h][ind, jyp, ix] + p4 * f[h][ind, jyp, ixp] for h in P.slot]
            out.append((v[0] * dt2 + v[1] * dt1) * dtt)
        return (dz1 * out[1] + dz2 * out[0]) * dz

    pvi, qvi, tti, uui, vvi, rhoi = (prof(f) for f in (P.pv, P.qv, P.tt, P.uu, P.vv, P.rho))
    tr = [h2(P.tropopause[h]) for h in P.slot]
    hm = [h2(P.hmix[h]) for h in P.slot]
    hmixi = (hm[0] * dt2 + hm[1] * dt1) * dtt
    tri = (tr[0] * dt2 + tr[1] * dt1) * dtt
    energy = tti * P.cpa + (zt + topo) * rt(9.81) + qvi * rt(2501000.) + (uui * uui + vvi * vvi) / rt(2.)
    xlon = xlon * P.pi180; ylat = ylat * P.pi180
    x = np.cos(ylat) * np.sin(xlon)
    y = rt(-1.) * np.cos(ylat) * np.cos(xlon)
    zc = np.sin(ylat)
    out = dict(cartx=x, carty=y, cartz=zc, z=zt, topo=topo, pv=pvi, qv=qvi, tt=tti, uu=uui, vv=vvi, rho=rhoi, tro=tri, hmix=hmixi, energy=energy)
    assert all(v.dtype == rt for v in out.values())
    return out


def accumulate(state, P, itime, xt, yt, zt, due, stats=None):
    """One pass of the particle loop: every particle with due[j] adds its values and counts the call (in place)."""
    due = np.asarray(due, bool)
    if not due.any():
        return state
    a = addends(P, itime, np.asarray(xt)[due], np.asarray(yt)[due], np.asarray(zt)[due], stats)
    for k in SUMS:
        state[k][due] = state[k][due] + a[k]
    state["npart_av"][due] += 1
    return state


def nint(v):
    """Fortran nint: to the nearest integer, halves away from zero (v - trunc(v) is exact)."""
    t = np.trunc(v)
    return (t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)).astype(np.int64)


SHORTS = ("xlon", "ylat", "z", "topo", "tro", "hmix", "rho", "qv", "pv", "tt", "uu", "vv")


def shorts(state, valid, kind, stats=None):
    """partoutput_average.f90:74-161 for the particles valid[j]: dict of the thirteen int16 arrays (energy included,
    which the reference computes but does not write), indexed like valid.nonzero()."""
    rt = RT[kind]
    pi180 = rt(3.14159265) / rt(180.)
    cnt = state["npart_av"][valid].astype(rt)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = {k: state[k][valid] / cnt for k in SUMS}
    xlon = np.arctan2(a["cartx"], rt(-1.) * a["carty"])
    ylat = np.arctan2(a["cartz"], np.sqrt(a["cartx"] * a["cartx"] + a["carty"] * a["carty"]))
    xlon = xlon / pi180; ylat = ylat / pi180
    hi, lo = xlon > rt(180.), xlon < rt(-180.)
    xlon = np.where(hi, xlon - rt(360.), xlon)
    xlon = np.where(lo, xlon + rt(360.), xlon)
    if stats is not None:
        stats["wrap"] = stats.get("wrap", 0) + int(hi.sum() + lo.sum())
    out = {"xlon": nint(xlon * rt(180.)), "ylat": nint(ylat * rt(360.))}

    def clamp(name, zlim):
        up, dn = zlim > rt(32766.), zlim < rt(-32766.)
        if stats is not None:
            stats["clamp_hi_" + name] = stats.get("clamp_hi_" + name, 0) + int(up.sum())
            stats["clamp_lo_" + name] = stats.get("clamp_lo_" + name, 0) + int(dn.sum())
        out[name] = nint(np.maximum(np.minimum(zlim, rt(32766.)), rt(-32766.)))

    clamp("z", a["z"] * rt(2.) - rt(32000.))
    clamp("topo", a["topo"] * rt(2.) - rt(32000.))
    clamp("tro", a["tro"] * rt(2.) - rt(32000.))
    clamp("hmix", a["hmix"] * rt(2.) - rt(32000.))
    clamp("rho", a["rho"] * rt(20000.) - rt(32000.))
    clamp("qv", a["qv"] * rt(1000000.) - rt(32000.))
    clamp("pv", a["pv"] * rt(100.))
    clamp("tt", (a["tt"] - rt(273.15)) * rt(300.))
    clamp("uu", a["uu"] * rt(200.))
    clamp("vv", a["vv"] * rt(200.))
    clamp("energy", (a["energy"] - rt(300000.)) / rt(30.))
    return {k: v.astype(np.int16) for k, v in out.items()}


def records(state, itra1, itime, kind, stats=None):
    """The [n][12] int16 records of partoutput_average for the particles with itra1 = itime (rows of the others: zero) and
    the validity mask; the state is zeroed in place as :172-186 does."""
    valid = np.asarray(itra1) == itime
    rec = np.zeros((valid.size, 12), np.int16)
    if valid.any():
        sh = shorts(state, valid, kind, stats)
        for c, k in enumerate(SHORTS):
            rec[valid, c] = sh[k]
    for k in SUMS:
        state[k][:] = 0
    state["npart_av"][:] = 0
    return rec, valid


def file_bytes(rec, valid):
    """Direct access, recl = 24, no markers: the file ends with the last valid record; holes are zero bytes."""
    if not valid.any():
        return b""
    last = int(np.nonzero(valid)[0][-1])
    return np.ascontiguousarray(rec[: last + 1]).astype("<i2").tobytes()


def caldate(juldate):
    """caldate.f90:42-78 -> (yyyymmdd, hhmiss); the arithmetic is integer or float64 in either build."""
    julday = int(juldate)
    if (juldate - julday) * 86400. >= 86399.5:
        juldate = float(julday + 1); julday = julday + 1
    igreg = 2299161
    if julday >= igreg:
        jalpha = int(((julday - 1867216) - 0.25) / 36524.25)
        ja = julday + 1 + jalpha - int(0.25 * jalpha)
    else:
        ja = julday
    jb = ja + 1524
    jc = int(6680. + ((jb - 2439870) - 122.1) / 365.25)
    jd = 365 * jc + int(0.25 * jc)
    je = int((jb - jd) / 30.6001)
    dd = jb - jd - int(30.6001 * je)
    mm = je - 1
    if mm > 12:
        mm = mm - 12
    yyyy = jc - 4715
    if mm > 2:
        yyyy = yyyy - 1
    if yyyy <= 0:
        yyyy = yyyy - 1
    frac = juldate - float(julday)
    hh = int(24. * frac)
    mi = int(1440. * frac - 60. * float(hh))
    ss = int(np.floor(86400. * frac - 3600. * float(hh) - 60. * float(mi) + 0.5))
    if ss == 60:
        ss = 0; mi = mi + 1
    if mi == 60:
        mi = 0; hh = hh + 1
    return 10000 * yyyy + 100 * mm + dd, 10000 * hh + 100 * mi + ss


def file_name(bdate, itime):
    d, t = caldate(float(bdate) + float(itime) / 86400.)
    return "partposit_average_%08d%06d" % (d, t)


def run_case(c, kind, stats=None):
    """synthetic.partavg_case() through both routines: per output interval (state before the output call, records,
    validity mask, file bytes, file name)."""
    P = Params(c, kind)
    st = new_state(int(c["npart"]), kind)
    res, ncall = [], 0
    for iv, times in enumerate(c["calls"]):
        for itime in times:
            accumulate(st, P, itime, c[f"xt{ncall}"], c[f"yt{ncall}"], c[f"zt{ncall}"], c[f"due{ncall}"], stats)
            ncall += 1
        before = {k: v.copy() for k, v in st.items()}
        rec, valid = records(st, c[f"itra1_{iv}"], c["outputs"][iv], kind, stats)
        res.append((before, rec, valid, file_bytes(rec, valid), file_name(c["bdate"], c["outputs"][iv])))
    return res


def params_from_scenario(sc, kind, nymax=None):
    return Params(sc, kind, nymax=nymax if nymax is not None else int(sc["grid"][1]))
