"""numpy restatement of plumetraj.f90:56-230 with clustering.f90, centerofmass.f90, distance.f90, distance2.f90 and mean of
mean_mod, in the reference's real kinds ('r4': float32, 'r8': float64), serial, in the reference's order.

Every operation is one IEEE operation on values of the host's real kind H, nothing is contracted; where the reference
mixes a double position with default reals the expression is formed in float64 and rounded on assignment.  A sum is
np.add.accumulate in H, which adds strictly one element after the other like the reference's loop.  sin, cos, acos and
atan2 are the C library's (libm through ctypes / math), the functions a flang binary calls: numpy's own vector versions
differ from them in the last bit.  The interpolation to the particle is partavg_ref.addends (plumetraj.f90:92-168 is the
code of partpos_average.f90 word for word).

Besides the records the restatement keeps, per release point, what the tests derive their bounds and their margins from:
the passes of the loop, numb, n and the sum of |t| of every sum, and the margin of every decision (see `new_stats`)."""
import ctypes
import ctypes.util
import math

import numpy as np

import partavg_ref as pr

RT = pr.RT
NCLUSTER = 5
NVAL = 14
COLS = ("xcenter", "ycenter", "zcenter", "topocenter", "hmixcenter", "tropocenter", "pvcenter", "rmsdist", "rms", "zrmsdist", "zrms",
        "hmixfract", "pvfract", "tropofract")
CCOLS = ("xclust", "yclust", "zclust", "fclust", "rmsclust")
# (i5,i8,2f9.4,4f8.1,f8.2,4f8.1,3f6.1,5(2f8.3,f7.0,f6.1,f8.1))
FMT = ((9, 4), (9, 4), (8, 1), (8, 1), (8, 1), (8, 1), (8, 2), (8, 1), (8, 1), (8, 1), (8, 1), (6, 1), (6, 1), (6, 1))
CFMT = ((8, 3), (8, 3), (7, 0), (6, 1), (8, 1))

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf"):
    getattr(_libm, _n).argtypes = [ctypes.c_float]
    getattr(_libm, _n).restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float


def _acos(v):
    return math.acos(v) if -1.0 <= v <= 1.0 else math.nan


def _vec(f, a, rt=np.float64):
    return np.array([f(float(v)) for v in np.asarray(a).ravel()], rt).reshape(np.shape(a))


class Lib:
    """sin, cos, atan2 of the real kind; dsin, dcos, dacos of double precision -- all the C library's."""

    def __init__(self, kind):
        self.rt = RT[kind]
        if kind == "r4":
            self.sin = lambda a: _vec(_libm.sinf, a, np.float32)
            self.cos = lambda a: _vec(_libm.cosf, a, np.float32)
            self.atan2 = lambda a, b: np.float32(_libm.atan2f(float(a), float(b)))
        else:
            self.sin = lambda a: _vec(math.sin, a)
            self.cos = lambda a: _vec(math.cos, a)
            self.atan2 = lambda a, b: np.float64(math.atan2(float(a), float(b)))
        self.dsin = lambda a: _vec(math.sin, a)
        self.dcos = lambda a: _vec(math.cos, a)
        self.dacos = lambda a: _vec(_acos, a)


def serial_sum(t, rt):
    """0. + t(1) + t(2) + ... in H, one after the other."""
    t = np.asarray(t).astype(rt)
    return rt(0.) if t.size == 0 else np.add.accumulate(t)[-1]


KLIB = 4.0        # sin, cos, atan2 of the real kind: the device's value and the C library's within KLIB eps_H of each other, relatively
KDP = 8.0         # the same for the double functions inside distance and distance2, in units of 2^-52


def new_stats():
    """Counters over all release points: inactive, empty, few (n < ncluster), empty_cluster, in_box2, in_box, pv_north,
    pv_south, guard; points[j] (j 1-based) holds per release point
      n, passes, numb
      sums     {name: (number of terms, sum of |t|, own error)}: own error = |the serial sum in H - the exactly rounded sum of
               the same terms|, the reference's own summation error
      cent     per pass l the error bound [rad] of the centroids that pass MEASURES DISTANCES TO (0 in pass 1: the seeds are
               copies of particle positions), from the own errors of the sums behind them and KLIB
      gap      per pass (smallest second-nearest minus nearest centroid distance of a particle [km], bound of a distance in
               that pass [km]); a particle whose two nearest distances are both exactly 0 (distance2's box on both sides) is
               left out: the box margins cover it, and equal distances go to the first cluster on every side; so is a
               centroid that is a bitwise copy of the nearest one (two equal seeds)
      box2     per pass (smallest distance of a (particle, centroid) pair from the edge of distance2's box [rad], cent)
      exit     per pass l > 1 one of ("exact", 0, 0): the centroids are bitwise those of the pass before, so the distances, the
               assignment and rms repeat and the ratio is exactly 0 whatever the order of the sums; ("nan", 0, 0): rms and
               rmsold are exactly 0 (every particle inside the box), the ratio is 0/0 and compares false; else
               ("soft", |ratio - 0.005|, bound of the ratio)
      box      (distance from the edge of distance's 0.03 degree box against the centre of mass [degrees], bound of the
               centre [degrees])
      print    per column the smallest distance of a printed value from a rounding boundary of its format"""
    return dict(points={}, inactive=0, empty=0, few=0, empty_cluster=0, in_box2=0, in_box=0, pv_north=0, pv_south=0, guard=0)


def own_error(t, s):
    return abs(float(s) - math.fsum(float(v) for v in np.asarray(t).ravel()))


def sum_entry(t, s):
    t = np.asarray(t)
    return (int(t.size), float(np.abs(t.astype(np.float64)).sum()), own_error(t, s))


def sum_bound(entry, rt):
    """(a): |the device's sum - the restatement's|: the reference's own error, the fp64 partials, one rounding to H"""
    n, sabs, own = entry
    return own + n * 2.0 ** -52 * sabs + float(np.finfo(rt).eps) / 2 * sabs


def angle_bound(xav, yav, zav, ex, ey, ez, rt):
    """(d): first-order error of atan2(xav, -yav) and atan2(zav, sqrt(xav^2 + yav^2)) [rad] from the errors of the means"""
    eps = float(np.finfo(rt).eps)
    xav, yav, zav = abs(float(xav)), abs(float(yav)), abs(float(zav))
    h2 = xav * xav + yav * yav
    h = math.sqrt(h2)
    dx = (yav * ex + xav * ey) / h2 + KLIB * eps * math.atan2(xav, yav)
    eh = (xav * ex + yav * ey) / h + eps * h
    dy = (h * ez + zav * eh) / (h2 + zav * zav) + KLIB * eps * math.atan2(zav, h)
    return max(dx, dy)


def dist_bound(cent, dmin_pos, dmax, rt):
    """(c): a distance [km] against a point known to `cent` rad: the shift of the point, acos near 1 for the smallest
    distance that is not 0, one rounding to H"""
    ang = max(dmin_pos, 1e-9) / 6371.2
    return 6371.2 * (2.0 * cent + KDP * 2.0 ** -52 / math.sin(min(ang, 1.0))) + float(np.finfo(rt).eps) * dmax


def _box_margin(a, b, B):
    """a, b >= 0 (float64 arrays): distance of the decision (a < B and b < B) from flipping."""
    inside = (a < B) & (b < B)
    m_in = np.minimum(B - a, B - b)
    m_out = np.maximum(np.where(a >= B, a - B, 0.0), np.where(b >= B, b - B, 0.0))
    return inside, np.where(inside, m_in, m_out)


def distance2(L, yl, xl, slat1, clat1, yc, xc):
    """distance2.f90:43-56 of the particles (radians, H) to one centroid -> (km in H, margin of the box decisions, in the box)"""
    rt = L.rt
    B = rt(0.0003)
    a, b = np.abs(yl - yc), np.abs(xl - xc)
    box = (a < B) & (b < B)
    slat2, clat2 = math.sin(float(yc)), math.cos(float(yc))
    cdlon = L.dcos((xl - xc).astype(np.float64))
    crd = slat1 * slat2 + clat1 * clat2 * cdlon
    d = (6.3712e6 * L.dacos(crd) / 1000.0).astype(rt)
    d[box] = rt(0.)
    _, m = _box_margin(a.astype(np.float64), b.astype(np.float64), float(B))
    return d, float(m.min()), int(box.sum())


def distance(L, yl, xl, yc, xc):
    """distance.f90:43-54 (degrees) -> (km in H, margin of the box decisions, in the box)"""
    rt = L.rt
    B = rt(0.03)
    dpr = 180.0 / 3.14159265358979
    a, b = np.abs(yl - yc), np.abs(xl - xc)
    box = (a < B) & (b < B)
    clat1, slat1 = L.dcos(yl.astype(np.float64) / dpr), L.dsin(yl.astype(np.float64) / dpr)
    clat2, slat2 = math.cos(float(yc) / dpr), math.sin(float(yc) / dpr)
    cdlon = L.dcos((xl - xc).astype(np.float64) / dpr)
    crd = slat1 * slat2 + clat1 * clat2 * cdlon
    d = (6.3712e6 * L.dacos(crd) / 1000.0).astype(rt)
    d[box] = rt(0.)
    _, m = _box_margin(a.astype(np.float64), b.astype(np.float64), float(B))
    return d, float(m.min()), int(box.sum())


def clustering(L, xl, yl, zl, K, st):
    """clustering.f90 for n >= K particles: xl, yl come back as the routine leaves them (radians and back)."""
    rt = L.rt
    eps = float(np.finfo(rt).eps)
    n = xl.size
    pi180 = rt(3.14159265) / rt(180.)
    xr, yr = xl * pi180, yl * pi180
    seeds = [(j * n) // K - 1 for j in range(1, K + 1)]
    xc, yc = xr[seeds].copy(), yr[seeds].copy()
    slat1, clat1 = L.dsin(yr.astype(np.float64)), L.dcos(yr.astype(np.float64))
    cy = L.cos(yr)
    x = cy * L.sin(xr)
    y = rt(-1.) * cy * L.cos(xr)
    z = L.sin(yr)
    rmsold = rt(-5.)
    cent = 0.0                                            # of the centroids this pass measures distances to
    drms_old = 0.0
    prev = None
    st.update(cent=[], gap=[], box2=[], exit=[])
    for l in range(1, 101):
        res = [distance2(L, yr, xr, slat1, clat1, yc[j], xc[j]) for j in range(K)]
        dist = np.stack([r[0] for r in res])
        st["box2"].append((min(r[1] for r in res), cent))
        st["n_box2"] += sum(r[2] for r in res)
        st["cent"].append(cent)
        dmin = np.full(n, rt(1.e10)); ncl = np.zeros(n, np.int64); found = np.zeros(n, bool)
        for j in range(K):
            better = dist[j] < dmin
            dmin = np.where(better, dist[j], dmin); ncl = np.where(better, j, ncl); found |= better
        st["guard"] += int((~found).sum())
        pos = dist[dist > 0]
        dbound = dist_bound(cent, float(pos.min()) if pos.size else 1.0, float(dist.max()), rt)
        twin = (xc[:, None] == xc[ncl][None, :]) & (yc[:, None] == yc[ncl][None, :])      # the chosen centroid and its bitwise copies
        other = np.where(twin, np.inf, dist.astype(np.float64))
        second = other.min(axis=0) if K > 1 else np.full(n, np.inf)
        counted = ~((second == 0.) & (dmin == 0.))
        if counted.any():
            st["gap"].append((float((second - dmin.astype(np.float64))[counted].min()), dbound))
        d2 = dmin * dmin
        s_all = serial_sum(d2, rt)
        rms = np.sqrt(s_all / rt(n))
        st["sums"]["rms"] = sum_entry(d2, s_all)
        # (d) for rms = sqrt(sum d^2 / n): the distances move by dbound each, the sum by its bound, two roundings
        drms = (dbound + sum_bound(st["sums"]["rms"], rt) / (2.0 * n * float(rms)) + eps * float(rms)) if rms > 0 else 0.0
        same = prev is not None and np.array_equal(prev[0], xc) and np.array_equal(prev[1], yc)
        prev = (xc.copy(), yc.copy())
        numb = np.bincount(ncl, minlength=K)
        rmsclust = np.zeros(K, rt)
        cent_new = 0.0
        st["sums"]["rmsclust"] = {}
        for j in range(K):
            if numb[j] > 0:
                m = ncl == j
                nb = rt(numb[j])
                sd = serial_sum(d2[m], rt)
                st["sums"]["rmsclust"][j] = sum_entry(d2[m], sd)
                rmsclust[j] = np.sqrt(sd / nb)
                sx, sy, sz = serial_sum(x[m], rt), serial_sum(y[m], rt), serial_sum(z[m], rt)
                xav, yav, zav = sx / nb, sy / nb, sz / nb
                # the terms differ by 2 KLIB eps relatively between the libraries (two functions and a product), the sums by (a)
                ex, ey, ez = [(sum_bound(sum_entry(t[m], sv), rt) + 2 * KLIB * eps * float(np.abs(t[m].astype(np.float64)).sum())) / float(nb) + eps * abs(float(av))
                              for t, sv, av in ((x, sx, xav), (y, sy, yav), (z, sz, zav))]
                xc[j] = L.atan2(xav, rt(-1.) * yav)
                yc[j] = L.atan2(zav, np.sqrt(xav * xav + yav * yav))
                cent_new = max(cent_new, angle_bound(xav, yav, zav, ex, ey, ez, rt))
            else:
                st["empty_cluster"] += 1
        st["passes"] = l
        if l > 1:
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.abs(rms - rmsold) / rmsold
            if np.isnan(ratio):
                assert rms == 0 and rmsold == 0
                st["exit"].append(("nan", 0.0, 0.0))
            elif same:
                assert ratio == 0
                st["exit"].append(("exact", 0.0, 0.0))
            else:
                rb = (drms + drms_old * float(rms) / float(rmsold)) / float(rmsold) + 2 * eps * float(ratio)
                st["exit"].append(("soft", abs(float(ratio) - float(rt(0.005))), rb))
            if ratio < rt(0.005):
                break
        rmsold = rms
        drms_old = drms
        cent = cent_new
    st["cent_final"] = cent_new
    st["drms"] = drms
    st["dbound"] = dbound
    xl2, yl2 = xr / pi180, yr / pi180
    zclust = np.zeros(K, rt)
    st["sums"]["zclust"] = {}
    for j in range(K):
        if numb[j] > 0:
            sz = serial_sum(zl[ncl == j], rt)
            st["sums"]["zclust"][j] = sum_entry(zl[ncl == j], sz)
            zclust[j] = sz / rt(numb[j])
    fclust = (rt(100.) * numb.astype(rt) / rt(n)).astype(rt)
    zdist = zl - zclust[ncl]
    zrms = serial_sum(zdist * zdist, rt)
    st["sums"]["zrms"] = sum_entry(zdist * zdist, zrms)
    st["zdist_max"] = float(np.abs(zdist).max())
    if zrms > rt(0.):
        zrms = np.sqrt(zrms / rt(n))
    st["numb"] = numb.astype(np.int64)
    st["nclust"] = ncl
    return xl2, yl2, xc / pi180, yc / pi180, zclust, fclust, rms, rmsclust, zrms


def fmt_f(v, w, d):
    """Fw.d of the exact binary value, ties to even; the optional zero dropped when the field is too narrow; asterisks."""
    v = float(v)
    if math.isnan(v):
        t = "NaN"
    elif math.isinf(v):
        t = "-Inf" if v < 0 else "Inf"
    else:
        t = ("%#.0f" % v) if d == 0 else ("%.*f" % (d, v))
    if len(t) > w:
        z = 1 if t.startswith("-") else 0
        if t[z:z + 2] == "0.":
            t = t[:z] + t[z + 1:]
    if len(t) > w:
        t = "*" * w
    return t.rjust(w)


def fmt_i(v, w):
    t = "%d" % int(v)
    return ("*" * w if len(t) > w else t).rjust(w)


def record_text(j, age, values):
    s = fmt_i(j, 5) + fmt_i(age, 8)
    for k in range(NVAL):
        s += fmt_f(values[k], *FMT[k])
    for c in range(NCLUSTER):
        for k in range(5):
            s += fmt_f(values[NVAL + 5 * c + k], *CFMT[k])
    return s + "\n"


def print_margin(v, d):
    """distance of v from the nearest value that prints differently with d decimals"""
    s = abs(float(v)) * 10.0 ** d
    return abs(s - math.floor(s) - 0.5) / 10.0 ** d


def run(src, kind, itime, K=NCLUSTER, stats=None):
    """plumetraj(itime) for the particle arrays and the fields of `src` (a scenario-shaped dict with ireleasestart,
    ireleaseend, lage): the list of records, each a dict of j, age, n, passes, numb, values (H, 14 + 5 K), clustered."""
    rt = RT[kind]
    L = Lib(kind)
    P = pr.Params(src, kind)
    stats = new_stats() if stats is None else stats
    xt, yt = np.asarray(src["xtra1"], np.float64), np.asarray(src["ytra1"], np.float64)
    zt = np.asarray(src["ztra1"]).astype(rt)
    itra1, npoint = np.asarray(src["itra1"]), np.asarray(src["npoint"])
    start, end = np.asarray(src["ireleasestart"], np.int64), np.asarray(src["ireleaseend"], np.int64)
    lage = int(np.asarray(src["lage"]).ravel()[-1])
    recs = []
    for j in range(1, start.size + 1):
        if abs(int(start[j - 1]) - itime) > lage:
            stats["inactive"] += 1
            continue
        who = np.nonzero((itra1 == itime) & (npoint == j))[0]
        n = who.size
        if n == 0:
            stats["empty"] += 1
            continue
        st = dict(n=n, sums={}, gap=[], exit=[], box2=[], cent=[], box=None, n_box2=0, n_box=0, guard=0,
                  empty_cluster=0, passes=0, numb=np.zeros(K, np.int64), print={})
        a = pr.addends(P, itime, xt[who], yt[who], zt[who])
        xl = (np.float64(P.xlon0) + xt[who] * np.float64(P.dx)).astype(rt)
        yl = (np.float64(P.ylat0) + yt[who] * np.float64(P.dy)).astype(rt)
        zl = zt[who]
        topo, pvi, hmixi, tri = a["topo"], a["pv"], a["hmix"], a["tro"]
        north = yl > rt(0.)
        pvflag = np.where(north, pvi < rt(2.), pvi > rt(-2.))
        stats["pv_north"] += int(north.sum()); stats["pv_south"] += int((~north).sum())
        rn = rt(n)
        val = np.zeros(NVAL + 5 * K, rt)
        tt = np.stack([tri, topo], axis=1).ravel()        # tropocenter=tropocenter+tri+topo, left to right
        for k, nm, t in ((3, "topocenter", topo), (4, "hmixcenter", hmixi), (6, "pvcenter", pvi), (5, "tropocenter", tt)):
            sv = serial_sum(t, rt)
            st["sums"][nm] = sum_entry(t, sv)
            val[k] = sv / rn
        val[11] = rt(100.) * rt((zl < hmixi).sum()) / rn
        val[12] = rt(100.) * rt(pvflag.sum()) / rn
        val[13] = rt(100.) * rt((zl < tri).sum()) / rn
        zl = zl + topo
        clustered = n >= K
        if clustered:
            xl, yl, xclust, yclust, zclust, fclust, rms, rmsclust, zrms = clustering(L, xl, yl, zl, K, st)
            val[8], val[10] = rms, zrms
            for c in range(K):
                val[NVAL + 5 * c: NVAL + 5 * c + 5] = (xclust[c], yclust[c], zclust[c], fclust[c], rmsclust[c])
        else:
            stats["few"] += 1
        pi180 = rt(3.14159265) / rt(180.)
        xll, yll = xl * pi180, yl * pi180
        cy = L.cos(yll)
        x = cy * L.sin(xll); y = rt(-1.) * cy * L.cos(xll); z = L.sin(yll)
        eps = float(np.finfo(rt).eps)
        sx, sy, sz = serial_sum(x, rt), serial_sum(y, rt), serial_sum(z, rt)
        xav, yav, zav = sx / rn, sy / rn, sz / rn
        ex, ey, ez = [(sum_bound(sum_entry(t, sv), rt) + 2 * KLIB * eps * float(np.abs(t.astype(np.float64)).sum())) / n + eps * abs(float(av))
                      for t, sv, av in ((x, sx, xav), (y, sy, yav), (z, sz, zav))]
        st["centre"] = angle_bound(xav, yav, zav, ex, ey, ez, rt)     # of the centre of mass [rad]
        val[0] = L.atan2(xav, rt(-1.) * yav) / pi180
        val[1] = L.atan2(zav, np.sqrt(xav * xav + yav * yav)) / pi180
        s1, s2 = serial_sum(zl, rt), serial_sum(zl * zl, rt)
        st["sums"]["z"] = sum_entry(zl, s1)
        st["sums"]["zq"] = sum_entry(zl * zl, s2)
        val[2] = s1 / rn
        xaux = s2 - s1 * s1 / rn
        st["xaux"] = float(xaux)
        val[9] = rt(0.) if xaux < rt(1.0e-30) else np.sqrt(xaux / rt(n - 1))
        dist, bm, nb = distance(L, yl, xl, val[1], val[0])
        centre_deg = st["centre"] / float(pi180) + eps * max(abs(float(val[0])), abs(float(val[1])))
        st["box"] = (bm, centre_deg)
        st["n_box"] = nb
        d2 = dist * dist
        rmsdist = serial_sum(d2, rt)
        st["sums"]["rmsdist"] = sum_entry(d2, rmsdist)
        st["dc_bound"] = dist_bound(st["centre"] + 2 * eps * float(np.abs(yl * pi180).max() + np.abs(xl * pi180).max()),
                                    float(dist[dist > 0].min()) if (dist > 0).any() else 1.0, float(dist.max()), rt)
        if rmsdist > rt(0.):
            rmsdist = np.sqrt(rmsdist / rn)
        val[7] = max(rmsdist, rt(0.))
        ncols = NVAL + 5 * K if clustered else NVAL
        fm = list(FMT) + list(CFMT) * K
        for k in range(ncols):
            if clustered or k not in (8, 10):
                name = COLS[k] if k < NVAL else CCOLS[(k - NVAL) % 5]
                st["print"][name] = min(st["print"].get(name, math.inf), print_margin(val[k], fm[k][1]))
        stats["in_box2"] += st["n_box2"]; stats["in_box"] += st["n_box"]
        stats["guard"] += st["guard"]; stats["empty_cluster"] += st["empty_cluster"]
        stats["points"][j] = st
        recs.append(dict(j=j, age=itime - int((int(start[j - 1]) + int(end[j - 1])) / 2), n=n, passes=st["passes"], numb=st["numb"], values=val,
                         clustered=clustered))
    return recs


def text(recs):
    return "".join(record_text(r["j"], r["age"], r["values"]) for r in recs)


def defined_columns(rec):
    """the byte ranges of a record's line the reference defines: everything for a clustered point; without rms, zrms and the
    cluster columns for a point with fewer particles than clusters"""
    widths = [5, 8] + [w for w, _ in FMT] + [w for w, _ in CFMT] * NCLUSTER
    pos = np.concatenate([[0], np.cumsum(widths)])
    keep = []
    for k in range(len(widths)):
        v = k - 2
        if rec["clustered"] or (v < NVAL and v not in (8, 10)):
            keep.append((int(pos[k]), int(pos[k + 1])))
    return keep


def column_bounds(rec, st, kind, K=NCLUSTER):
    """Per value of a record (the order of rec["values"]) the bound of |the device's value - the restatement's| of DESIGN
    section 21, from the statistics `st` of the release point alone: (a) the reference's own summation error, the fp64
    partials and one rounding; (b) KLIB eps_H between the libraries; (c) acos near 1; (d) first-order propagation through
    atan2, sqrt and mean's cancelling xq - xl^2/n.  0: the value is integer-derived and must be equal.  nan: not compared
    (the columns the reference leaves undefined for n < ncluster)."""
    rt = RT[kind]
    eps = float(np.finfo(rt).eps)
    v = rec["values"].astype(np.float64)
    n = rec["n"]
    S = st["sums"]
    b = np.zeros(v.size)
    for k, nm in ((3, "topocenter"), (4, "hmixcenter"), (6, "pvcenter"), (5, "tropocenter"), (2, "z")):
        b[k] = sum_bound(S[nm], rt) / n + eps * abs(v[k])
    pi180 = float(rt(3.14159265) / rt(180.))
    b[0] = b[1] = st["centre"] / pi180 + eps * max(abs(v[0]), abs(v[1]))
    s1, s2 = v[2] * n, S["zq"][1]
    dxaux = sum_bound(S["zq"], rt) + 2.0 * abs(s1) * sum_bound(S["z"], rt) / n + 2.0 * eps * (s2 + s1 * s1 / n)
    b[9] = dxaux / (2.0 * v[9] * (n - 1)) + eps * v[9] if v[9] > 0 else math.sqrt(dxaux / max(n - 1, 1))
    b[7] = st["dc_bound"] + (sum_bound(S["rmsdist"], rt) / (2.0 * n * v[7]) + eps * v[7] if v[7] > 0 else 0.0)
    if not rec["clustered"]:
        b[8] = b[10] = math.nan
        b[NVAL:] = math.nan
        return b
    b[8] = st["drms"]
    dz = {j: sum_bound(e, rt) / e[0] + eps * abs(v[NVAL + 5 * j + 2]) for j, e in S["zclust"].items()}
    b[10] = max(dz.values()) + (sum_bound(S["zrms"], rt) / (2.0 * n * v[10]) + eps * v[10] if v[10] > 0 else 0.0)
    for j in range(K):
        c = NVAL + 5 * j
        b[c] = b[c + 1] = st["cent_final"] / pi180 + eps * max(abs(v[c]), abs(v[c + 1]))
        b[c + 2] = dz.get(j, 0.0)
        e = S["rmsclust"].get(j)
        if e is not None:
            b[c + 4] = st["dbound"] + (sum_bound(e, rt) / (2.0 * e[0] * v[c + 4]) + eps * v[c + 4] if v[c + 4] > 0 else 0.0)
    return b
