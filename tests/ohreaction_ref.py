"""numpy restatement of gethourlyOH.f90:40-142 (with caldate.f90, zenithangle.f90, photo_O1D.f90) and ohreaction.f90:47-153 in
both real kinds, operation by operation in the reference's order.  sin, cos, asin, exp, log and pow are the C library's through
ctypes, the functions a flang binary calls; numpy's own vector versions differ from them in the last bit.

Besides the results it records every discrete decision: the branch of gethourlyOH, and per particle the nest, ix, jy, indz, n,
OHx, OHy, OHz, both tiny tests, nearest-index ties and the particles with no level above them.

TEST INFRASTRUCTURE ONLY: checked against flang builds of the unmodified routines (tests/golden/oh_r4.npz, oh_r8.npz)."""
import ctypes
import ctypes.util

import numpy as np

RT = {"r4": np.float32, "r8": np.float64}
DEAD = -999999999
BR_NONE, BR_ADVANCE, BR_INIT = 0, 1, 2

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sin", "cos", "asin", "exp", "log"):
    getattr(_libm, _n).argtypes = [ctypes.c_double]
    getattr(_libm, _n).restype = ctypes.c_double
    getattr(_libm, _n + "f").argtypes = [ctypes.c_float]
    getattr(_libm, _n + "f").restype = ctypes.c_float
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
_libm.pow.restype = ctypes.c_double
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.powf.restype = ctypes.c_float


class Libm:
    """libm in the real kind rt, elementwise."""

    def __init__(self, rt):
        self.rt = rt
        sfx = "f" if rt is np.float32 else ""
        for n in ("sin", "cos", "asin", "exp", "log", "pow"):
            setattr(self, "_" + n, getattr(_libm, n + sfx))

    def _map(self, fn, *a):
        a = np.broadcast_arrays(*[np.asarray(x, self.rt) for x in a])
        out = np.empty(a[0].shape, self.rt)
        flat = [x.ravel() for x in a]
        o = out.ravel()
        for i in range(o.size):
            o[i] = fn(*[float(x[i]) for x in flat])
        return out if out.shape else self.rt(out)

    def sin(self, a): return self._map(self._sin, a)
    def cos(self, a): return self._map(self._cos, a)
    def asin(self, a): return self._map(self._asin, a)
    def exp(self, a): return self._map(self._exp, a)
    def log(self, a): return self._map(self._log, a)
    def pow(self, a, b): return self._map(self._pow, a, b)


def caldate(juldate, rt):
    """caldate.f90:42-78 -> (juldate as the routine leaves it, yyyymmdd, hhmiss); the default-kind arithmetic in rt."""
    juldate = np.float64(juldate)
    julday = int(juldate)
    if (juldate - np.float64(julday)) * np.float64(86400.) >= np.float64(86399.5):
        juldate = juldate + juldate - np.float64(julday) - np.float64(86399.5) / np.float64(86400.)
        julday = int(juldate)
    if julday >= 2299161:
        jalpha = int((rt(julday - 1867216) - rt(0.25)) / rt(36524.25))
        ja = julday + 1 + jalpha - int(rt(0.25) * rt(jalpha))
    else:
        ja = julday
    jb = ja + 1524
    jc = int(rt(6680.) + (rt(jb - 2439870) - rt(122.1)) / rt(365.25))
    jd = 365 * jc + int(rt(0.25) * rt(jc))
    je = int(rt(jb - jd) / rt(30.6001))
    dd = jb - jd - int(rt(30.6001) * rt(je))
    mm = je - 1
    if mm > 12:
        mm -= 12
    yyyy = jc - 4715
    if mm > 2:
        yyyy -= 1
    if yyyy <= 0:
        yyyy -= 1
    fr = juldate - np.float64(julday)
    hh = int(np.float64(24.) * fr)
    mi = int(np.float64(1440.) * fr - np.float64(60.) * np.float64(hh))
    sec = np.float64(86400.) * fr - np.float64(3600.) * np.float64(hh) - np.float64(60.) * np.float64(mi)
    ss = int(np.floor(sec + 0.5)) if sec >= 0 else -int(np.floor(-sec + 0.5))       # nint
    if ss == 60:
        ss = 0; mi += 1
    if mi == 60:
        mi = 0; hh += 1
    return juldate, 10000 * yyyy + 100 * mm + dd, 10000 * hh + 100 * mi + ss


def month_of(yyyymmdd):
    return (yyyymmdd - (yyyymmdd // 10000) * 10000) // 100


def zenithangle(ylat, xlon, jul, rt, lm):
    """zenithangle.f90:44-74 for arrays ylat, xlon (kind rt) -> (sza, jul as caldate leaves it)."""
    jul, ymd, hms = caldate(jul, rt)
    jjjj = ymd // 10000
    mm = ymd // 100 - jjjj * 100
    idd = ymd - jjjj * 10000 - mm * 100
    iu = hms // 10000
    minute = hms // 100 - 100 * iu
    ndaynum = 31 * (mm - 1) + idd
    if mm > 2:
        ndaynum -= int(rt(0.4) * rt(mm) + rt(2.3))
    if mm > 2 and jjjj // 4 * 4 == jjjj:
        ndaynum += 1
    pi = rt(3.1415927)
    rnum = rt(2.) * pi * rt(ndaynum) / rt(365.)
    rylat = pi * ylat / rt(180.)
    ttime = rt(iu) + rt(minute) / rt(60.)
    s1, s2, s3, s4 = lm.sin(rnum), lm.sin(rt(2.) * rnum), lm.sin(rt(3.) * rnum), lm.sin(rt(4.) * rnum)
    c1, c2, c3, c4 = lm.cos(rnum), lm.cos(rt(2.) * rnum), lm.cos(rt(3.) * rnum), lm.cos(rt(4.) * rnum)
    dekl = rt(0.396) + rt(3.631) * s1 + rt(0.038) * s2 + rt(0.077) * s3 - rt(22.97) * c1 - rt(0.389) * c2 - rt(0.158) * c3
    rdekl = pi * dekl / rt(180.)
    eq = (rt(0.003) - rt(7.343) * s1 - rt(9.47) * s2 - rt(0.329) * s3 - rt(0.196) * s4 + rt(0.552) * c1 - rt(3.020) * c2 -
          rt(0.076) * c3 - rt(0.125) * c4) / rt(60.)
    sinsol = lm.sin(rylat) * lm.sin(rdekl) + lm.cos(rylat) * lm.cos(rdekl) * lm.cos((ttime - rt(12.) + xlon / rt(15.) + eq) * pi / rt(12.))
    solelev = lm.asin(sinsol) * rt(180.) / pi
    return rt(90.) - solelev, jul


ZANGLE = (0., 10., 20., 30., 40., 50., 60., 70., 78., 86., 90.0001)
FACT_PHOTO = (0.4616E-02, 0.4478E-02, 0.4131E-02, 0.3583E-02, 0.2867E-02, 0.2081E-02, 0.1235E-02, 0.5392E-03, 0.2200E-03, 0.1302E-03, 0.0902E-03)


def photo_O1D(sza, rt, lm):
    """photo_O1D.f90:38-56 for an array of zenith angles."""
    sza = np.asarray(sza, rt)
    za = np.array(ZANGLE, np.float64).astype(rt)
    fp = np.array(FACT_PHOTO, np.float64).astype(rt)
    pi = rt(3.1415927)
    out = np.zeros(sza.shape, rt)
    lit = sza < rt(90.)
    if not lit.any():
        return out
    s = sza[lit]
    ik = np.zeros(s.shape, np.int64)
    for iz in range(10):
        ik = np.where(s >= za[iz], iz, ik)
    z1 = rt(1.) / lm.cos(za[ik] * pi / rt(180.))
    z2 = rt(1.) / lm.cos(za[ik + 1] * pi / rt(180.))
    zg = rt(1.) / lm.cos(s * pi / rt(180.))
    dummy = (zg - z1) / (z2 - z1)
    f1 = lm.log(fp[ik])
    f2 = lm.log(fp[ik + 1])
    photo_no2 = rt(1.45e-2) * lm.exp(rt(-0.4) / lm.cos(s * pi / rt(180.)))
    out[lit] = photo_no2 * lm.exp(f1 + (f2 - f1) * dummy)
    return out


def nearest(a, x):
    """minloc(abs(a - x)) per x, 0-based (the first index of the minimum), and whether the minimum is attained twice."""
    d = np.abs(a[None, :] - np.asarray(x)[:, None])
    idx = d.argmin(axis=1)
    ties = (d == d.min(axis=1)[:, None]).sum(axis=1) > 1
    return idx, ties


def alt_tops(alt):
    """altOHtop of ohreaction.f90:114-117."""
    rt = alt.dtype.type
    top = np.empty_like(alt)
    top[:-1] = alt[1:] + rt(0.5) * (alt[1:] - alt[:-1])
    top[-1] = alt[-1] + rt(0.5) * (alt[-1] - alt[-2])
    return top


class OH:
    """oh_mod and what the two routines read of com_mod, in one real kind, for flexpart_amd.synthetic.oh_case()."""

    def __init__(self, c, kind):
        self.kind, self.rt = kind, RT[kind]
        rt = self.rt
        self.lm = Libm(rt)
        self.c = c
        self.ldirect = int(c["ldirect"])
        self.bdate = np.float64(c["bdate"])
        for k in ("lonOH", "latOH", "altOH", "OH_field", "jrate_average", "lonjr", "latjr", "height", "tt"):
            setattr(self, k, np.asarray(c[k]).astype(rt))
        self.nxo, self.nyo, self.nzo = (int(v) for v in c["ohgrid"])
        self.hourly = np.zeros((2, self.nzo, self.nyo, self.nxo), rt)
        self.memtime = np.zeros(2, rt)
        self.ijx, _ = nearest(self.lonjr, self.lonOH)
        self.jjy, _ = nearest(self.latjr, self.latOH)
        self.branches = []

    def _field(self, jul, m):
        rt = self.rt
        lat, lon = np.meshgrid(self.latOH, self.lonOH, indexing="ij")
        sza, jul = zenithangle(lat, lon, jul, rt, self.lm)
        jrate = photo_O1D(sza, rt, self.lm)
        ja = self.jrate_average[m - 1][self.jjy[:, None], self.ijx[None, :]]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.OH_field[m - 1] * jrate[None] / ja[None]
        return np.where(ja[None] > rt(0.), v, rt(0.)).astype(rt), sza

    def gethourlyOH(self, itime):
        rt = self.rt
        ld, t = rt(self.ldirect), rt(self.ldirect * int(itime))
        mt = self.memtime
        if ld * mt[0] <= t and ld * mt[1] > t:
            br = BR_NONE
        elif ld * mt[1] <= t and mt[1] != rt(0.):
            mt[0] = mt[1]
            mt[1] = mt[0] + ld * rt(3600.)
            self.hourly[0] = self.hourly[1]
            jul2 = self.bdate + np.float64(mt[1]) / np.float64(86400.)
            jul2, ymd, _ = caldate(jul2, rt)
            self.hourly[1], self.sza2 = self._field(jul2, month_of(ymd))
            br = BR_ADVANCE
        else:
            jul1, ymd, _ = caldate(self.bdate, rt)
            m1 = month_of(ymd)
            mt[0] = rt(0.)
            jul2 = self.bdate + np.float64(self.ldirect) * np.float64(rt(1.) / rt(24.))
            jul2, ymd, _ = caldate(jul2, rt)
            m2 = month_of(ymd)
            mt[1] = ld * rt(3600.)
            self.hourly[0], self.sza1 = self._field(jul1, m1)
            self.hourly[1], self.sza2 = self._field(jul2, m2)
            self.months = (m1, m2)
            br = BR_INIT
        self.branches.append(br)
        return br

    def blend(self, itime):
        """ohreaction.f90:124-126 for every cell."""
        rt = self.rt
        return self.hourly[0] + (self.hourly[1] - self.hourly[0]) * (rt(int(itime)) - self.memtime[0]) / (self.memtime[1] - self.memtime[0])

    def ohreaction(self, itime, ltsample, memtime, xt, yt, zt, itra1, xmass1, rec=None):
        """ohreaction.f90:61-153 over all storage spaces (dead ones included, as the reference does) -> the new xmass1 [nspec][n]
        (kind rt).  rec: dict that receives the per-particle decisions."""
        rt, lm, c = self.rt, self.lm, self.c
        nx, ny, nz = (int(v) for v in c["grid"])
        dx, dy, xlon0, ylat0 = (rt(v) for v in c["geom"])
        xt, yt = np.asarray(xt, np.float64), np.asarray(yt, np.float64)
        zt = np.asarray(zt).astype(rt)
        n = xt.size
        nxn, nyn = c["nest"]
        dxn, dyn, xlon0n, ylat0n = (rt(v) for v in c["nestgeom"])
        xresoln, yresoln = dx / dxn, dy / dyn                                         # gridcheck_nests.f90:359-372
        xln, yln = (xlon0n - xlon0) / dx, (ylat0n - ylat0) / dy
        xrn, yrn = (xlon0n + rt(nxn - 1) * dxn - xlon0) / dx, (ylat0n + rt(nyn - 1) * dyn - ylat0) / dy
        inn = (xt > np.float64(xln)) & (xt < np.float64(xrn)) & (yt > np.float64(yln)) & (yt < np.float64(yrn))
        xtn = ((xt - np.float64(xln)) * np.float64(xresoln)).astype(rt)
        ytn = ((yt - np.float64(yln)) * np.float64(yresoln)).astype(rt)
        ix = np.where(inn, xtn.astype(np.int64), xt.astype(np.int64))
        jy = np.where(inn, ytn.astype(np.int64), yt.astype(np.int64))
        interp_time = rt(int(itime)) - rt(0.5) * rt(int(ltsample))
        interp_time = int(np.floor(interp_time + rt(0.5))) if interp_time >= 0 else -int(np.floor(-interp_time + rt(0.5)))
        nslot = 1 if abs(int(memtime[0]) - interp_time) < abs(int(memtime[1]) - interp_time) else 2
        above = self.height[None, 1:] > zt[:, None]                                   # :89-95
        nolevel = ~above.any(axis=1)
        indz = np.where(nolevel, nz - 1, above.argmax(axis=1) + 1)                    # no level above: the engine's clamp (counted)
        xlon = (xt * np.float64(dx) + np.float64(xlon0)).astype(rt)
        wrapped = xlon > rt(180.)
        xlon = np.where(wrapped, xlon - rt(360.), xlon).astype(rt)
        ylat = (yt * np.float64(dy) + np.float64(ylat0)).astype(rt)
        ohx, tx = nearest(self.lonOH, xlon)
        ohy, ty = nearest(self.latOH, ylat)
        top = alt_tops(self.altOH)
        ohz, _ = nearest(top, zt)                                                     # never nzOH: altOHtop(nzOH) = altOHtop(nzOH-1) ...
        _, tz = nearest(top[:-1], zt)                                                 # ... a tie the first-index rule always settles
        oh_average = self.blend(itime)[ohz, ohy, ohx]
        tiny = np.finfo(rt).tiny
        react = oh_average > tiny
        outside = (ix < 0) | (ix >= nx) | (jy < 0) | (jy >= ny)
        temp = self.tt[nslot - 1][indz - 1, np.clip(jy, 0, ny - 1), np.clip(ix, 0, nx - 1)]
        out = np.asarray(xmass1).astype(rt).copy()
        zeroed = np.zeros(out.shape, bool)
        rates = np.zeros(out.shape, np.float64)
        tl = rt(abs(int(ltsample)))
        for k in range(out.shape[0]):
            cc, dc, nc = rt(c["ohcconst"][k]), rt(c["ohdconst"][k]), rt(c["ohnconst"][k])
            if not cc > rt(0.):
                continue
            t = temp[react]
            ohrate = cc * lm.pow(t, nc) * lm.exp(-dc / t) * oh_average[react]
            restmass = out[k, react] * lm.exp(rt(-1.) * ohrate * tl)
            keep = restmass > tiny
            out[k, react] = np.where(keep, restmass, rt(0.))
            zeroed[k, react] = ~keep
            rates[k, react] = ohrate.astype(np.float64)
        if rec is not None:
            rec.update(ngrid=inn.astype(np.int32), ix=ix, jy=jy, indz=indz, n=nslot, ohx=ohx, ohy=ohy, ohz=ohz, react=react, zeroed=zeroed,
                       ties=tx | ty | tz, nolevel=nolevel, outside=outside, wrapped=wrapped, temp=temp.astype(np.float64),
                       oh=oh_average.astype(np.float64), rates=rates, live=np.asarray(itra1) != DEAD)
        return out


def run_case(c, kind, masses):
    """The call sequence of oh_case(): per call a dict -- 'hourly': branch, OH_hourly, memOHtime; 'react': xmass1 and the record."""
    o = OH(c, kind)
    res = []
    m = np.asarray(masses).astype(RT[kind])
    for call in c["calls"]:
        if call[0] == "hourly":
            br = o.gethourlyOH(call[1])
            res.append(dict(kind="hourly", branch=br, OH_hourly=o.hourly.copy(), memOHtime=o.memtime.copy()))
        else:
            _, itime, lts, mt, mi = call
            rec = {}
            m = o.ohreaction(itime, lts, mt, c["xtra1"], c["ytra1"], c["ztra1"], c["itra1"], m, rec)
            res.append(dict(kind="react", xmass1=m.copy(), rec=rec, itime=itime, ltsample=lts, memtime=mt, memind=mi, blend=o.blend(itime)))
    return res, o
