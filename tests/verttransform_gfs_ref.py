"""numpy restatement of verttransform_gfs.f90:84-494 (NCEP GFS pressure levels -> z levels; without the cloud block
:498-596) in a given real kind.  Every column goes through the reference's loops in the reference's order -- llev, the height
recursion, pinmconv, the u/v sweep, the w sweep, drhodz, then the slope sweep, then the polar caps -- with the same
expressions; the columns are advanced together (numpy over the horizontal grid, Python loops over iz and kz), which changes no
value because no statement of a column reads what another column computed except the slope term's uvwzlev and the one carried
state the record counts (below).  log, cos, sin, atan and 10**x are the C library's through ctypes, the functions a flang
binary calls; numpy's own vector versions differ from them in the last bit.

State that outlives a call, as in the reference: height and nmixz (set by the first call), and ww of each of the two slots
(com_mod; zero at start): the w sweep :274-285 writes a z level only where it finds a bracket, so a level 2..nz-1 above the
column's top keeps the slot's old value and the slope term :354 is added to that.

uvwzlev is an automatic array of the routine: every call starts with it NaN here.  The slope term reads the neighbours'
uvwzlev at the centre's bracket levels; next to a step in llev that can be an entry the routine never wrote.  Those ww cells
come out NaN -- that is the mask the tests apply (and the pole row's zonal mean over a ring with such a cell).

The record `rec` of a call:
  llev_hist[k]        number of columns with llev = k (index 0 unused)
  llev                [ny][nx]
  above_uv, above_w   z levels 2..nz-1 above the column's top in the u/v sweep (:229) / without bracket in the w sweep (:276)
  w_top_swept         columns whose ww(nz) the w sweep overwrote (:274 runs to nz)
  tv_big, tv_small    outcomes of |tv - tvold| > 0.2 in the column recursion (:174)
  carried             slope terms computed with the bracket of an earlier z level of the column (:329-339 found none)
  carry_across        columns whose z level 2 found no bracket in the slope sweep: the reference would use the previous
                      column's bracket there; the restatement leaves NaN.  The test inputs must have none.
  margin              the smallest |height(iz) - uvwzlev(nuvz)| / uvwzlev(nuvz) over all columns and z levels 2..nz
  masked              number of NaN cells of ww
"""
import ctypes
import ctypes.util

import numpy as np

KINDS = {"r4": np.float32, "r8": np.float64}
FIELDS = ("uu", "vv", "ww", "tt", "qv", "pv", "rho", "drhodz", "pplev")
SWITCHNORTH, SWITCHSOUTH = 75.0, -75.0      # par_mod.f90:123

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("log", "cos", "sin", "atan"):
    getattr(_libm, _n).argtypes = [ctypes.c_double]
    getattr(_libm, _n).restype = ctypes.c_double
    getattr(_libm, _n + "f").argtypes = [ctypes.c_float]
    getattr(_libm, _n + "f").restype = ctypes.c_float
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
_libm.pow.restype = ctypes.c_double
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.powf.restype = ctypes.c_float


class Math:
    """libm in real kind H, elementwise over arrays; dsin / dcos always in double (cmapf_mod's internals)."""

    def __init__(self, H):
        self.H = H
        sfx = "f" if H is np.float32 else ""
        self._f = {n: getattr(_libm, n + sfx) for n in ("log", "cos", "sin", "atan", "pow")}

    def _vec(self, fn, a, H=None):
        H = H or self.H
        a = np.asarray(a)
        return np.array([fn(float(x)) for x in a.ravel()], H).reshape(a.shape)

    def log(self, a): return self._vec(self._f["log"], a)
    def cos(self, a): return self._vec(self._f["cos"], a)
    def sin(self, a): return self._vec(self._f["sin"], a)
    def atan(self, a): return self._vec(self._f["atan"], a)
    def pow10(self, a): return self.H(self._f["pow"](10.0, float(a)))
    def dsin(self, a): return self._vec(_libm.sin, a, np.float64)
    def dcos(self, a): return self._vec(_libm.cos, a, np.float64)


def new_state():
    return {"height": None, "nmixz": None, "ww": {}}


def llev_of(ps, akz):
    """verttransform_gfs.f90:149-154, [ny][nx] (1-based level numbers)"""
    nuvz = len(akz)
    llev = np.zeros(ps.shape, np.int64)
    for i in range(1, nuvz + 1):
        llev = np.where(ps < akz[i - 1], i, llev)
    return np.minimum(llev + 1, nuvz - 2)


def _ew(M, x):
    """ew.f90:4-29"""
    H = M.H
    y = H(373.16) / x
    a = H(-7.90298) * (y - H(1.))
    a = a + (H(5.02808) * H(0.43429) * M.log(y))
    c = (H(1.) - (H(1.) / y)) * H(11.344)
    c = H(-1.) + M.pow10(c)
    c = H(-1.3816) * c / H(1.e7)
    d = (H(1.) - y) * H(3.49149)
    d = H(-1.) + M.pow10(d)
    d = H(8.1328) * d / H(1.e3)
    y = a + c + d
    return H(101324.6) * M.pow10(y)


def _cc2gll(M, s, xlat, xlong, ue, vn):
    """cmapf_mod.f90:24-52 with cspanf :494-524; s = the map's nine reals; xlat scalar, xlong / ue / vn arrays"""
    H = M.H
    radpdg = H(3.14159265358979) / H(180.)
    first, last = H(-180.), H(180.)
    val = np.fmod(xlong - s[1] - first, last - first).astype(H)
    along = np.where(val <= H(0.), val + last, val + first).astype(np.float64)
    if xlat > H(89.985):
        rot = -np.float64(s[0]) * along + xlong.astype(np.float64) - 180.
    elif xlat < H(-89.985):
        rot = -np.float64(s[0]) * along - xlong.astype(np.float64)
    else:
        rot = -np.float64(s[0]) * along
    slong, clong = M.dsin(np.float64(radpdg) * rot), M.dcos(np.float64(radpdg) * rot)
    xpolg = slong * np.float64(s[4]) + clong * np.float64(s[5])
    ypolg = clong * np.float64(s[4]) - slong * np.float64(s[5])
    ue, vn = ue.astype(np.float64), vn.astype(np.float64)
    return (ypolg * ue + xpolg * vn).astype(H), (ypolg * vn - xpolg * ue).astype(H)


def polar_rows(m):
    """rows on which uupol / vvpol are defined (verttransform_gfs.f90:367,436), for either real kind"""
    ny = int(m["grid"][1])
    dy, ylat0 = float(m["geom"][1]), float(m["geom"][3])
    rows = np.zeros(ny, bool)
    if int(m["globalflags"][1]):
        rows[max(0, int((SWITCHNORTH - ylat0) / dy) - 2):] = True
    if int(m["globalflags"][2]):
        rows[: int((SWITCHSOUTH - ylat0) / dy) + 3 + 1] = True
    return rows


def vtgfs_ref(m, kind, state, slot, init=False, polemaps=None):
    """One call verttransform_gfs(slot, uuh, vvh, wwh, pvh) on a synthetic.gfs_levels() dict.  state: new_state(), carried from
    call to call.  polemaps = (northpolemap[9], southpolemap[9]) for a grid with polar caps.  Returns (fields, rec): float64
    arrays [nz][ny][nx] of FIELDS (+ uupol, vvpol), height, nmixz."""
    H = KINDS[kind]
    M = Math(H)
    nx, ny, nz = (int(v) for v in m["grid"])
    nuvz = nwz = nz
    dx, dy, xlon0, ylat0 = (H(v) for v in m["geom"])
    nglobal, sglobal = bool(m["globalflags"][1]), bool(m["globalflags"][2])
    akz, bkz, aknew, bknew = (np.asarray(m[k]).astype(H) for k in ("akz", "bkz", "aknew", "bknew"))
    ps, tt2, td2 = (np.asarray(m[k]).astype(H) for k in ("ps", "tt2", "td2"))
    tth, qvh, uuh, vvh, wwh, pvh = (np.asarray(m[k]).astype(H) for k in ("tth", "qvh", "uuh", "vvh", "wwh", "pvh"))
    pi, r_earth, r_air, ga = H(3.14159265), H(6.371e6), H(287.05), H(9.81)
    pi180 = pi / H(180.)
    const = r_air / ga
    dxconst = H(180.) / (dx * r_earth * pi)            # gridcheck_gfs.f90:241-242
    dyconst = H(180.) / (dy * r_earth * pi)
    rec = {}

    # ---- :84-139 ----
    if init or state["height"] is None:
        jj, ii = np.nonzero(ps > H(100000.))
        jym, ixm = int(jj[0]), int(ii[0])              # first in (jy, ix) order
        p0 = ps[jym, ixm]
        tvold = tt2[jym, ixm] * (H(1.) + H(0.378) * _ew(M, td2[jym, ixm]) / p0)
        pold = p0
        height = np.zeros(nz, H)
        for kz in range(2, nuvz + 1):
            pint = akz[kz - 1] + bkz[kz - 1] * p0
            tv = tth[kz - 1, jym, ixm] * (H(1.) + H(0.608) * qvh[kz - 1, jym, ixm])
            if abs(tv - tvold) > H(0.2):
                height[kz - 1] = height[kz - 2] + const * M.log(pold / pint) * (tv - tvold) / M.log(tv / tvold)
            else:
                height[kz - 1] = height[kz - 2] + const * M.log(pold / pint) * tv
            tvold, pold = tv, pint
        nmixz = nz
        for kz in range(1, nz + 1):
            if height[kz - 1] > H(4500.):
                nmixz = kz
                break
        state["height"], state["nmixz"] = height, nmixz
    height = state["height"]

    def take(A, K):
        return np.take_along_axis(A, (K - 1)[None], 0)[0]

    # ---- :145-198 ----
    llev = llev_of(ps, akz)
    rec["llev"] = llev
    rec["llev_hist"] = np.bincount(llev.ravel(), minlength=nuvz + 1)
    U = np.full((nz, ny, nx), np.nan, H)               # uvwzlev (wzlev is the same numbers)
    rhoh = np.full((nz, ny, nx), np.nan, H)
    tvold = take(tth, llev) * (H(1.) + H(0.608) * take(qvh, llev))
    pold = akz[llev - 1]
    np.put_along_axis(U, (llev - 1)[None], H(0.), 0)
    np.put_along_axis(rhoh, (llev - 1)[None], (pold / (r_air * tvold))[None], 0)
    rec["tv_big"] = rec["tv_small"] = 0
    for kz in range(2, nuvz + 1):
        a = kz >= llev + 1
        if not a.any():
            continue
        pint = akz[kz - 1] + bkz[kz - 1] * ps[a]
        tv = tth[kz - 1][a] * (H(1.) + H(0.608) * qvh[kz - 1][a])
        rhoh[kz - 1][a] = pint / (r_air * tv)
        big = np.abs(tv - tvold[a]) > H(0.2)
        lp = M.log(pold[a] / pint)
        new = np.empty(tv.shape, H)
        new[big] = U[kz - 2][a][big] + const * lp[big] * (tv[big] - tvold[a][big]) / M.log(tv[big] / tvold[a][big])
        new[~big] = U[kz - 2][a][~big] + const * lp[~big] * tv[~big]
        U[kz - 1][a] = new
        rec["tv_big"] += int(big.sum()); rec["tv_small"] += int((~big).sum())
        tvold[a] = tv
        pold = np.where(a, akz[kz - 1] + bkz[kz - 1] * ps, pold)
    assert U.dtype == H and rhoh.dtype == H

    def pk(k):                                         # aknew(k)+bknew(k)*ps, k scalar or [ny][nx], 1-based
        return aknew[k - 1] + bknew[k - 1] * ps
    pinm = np.full((nz, ny, nx), np.nan, H)
    np.put_along_axis(pinm, (llev - 1)[None], ((take(U, llev + 1) - take(U, llev)) / (pk(llev + 1) - pk(llev)))[None], 0)
    for kz in range(2, nz):
        a = kz >= llev + 1
        pinm[kz - 1][a] = ((U[kz] - U[kz - 2]) / (pk(kz + 1) - pk(kz - 1)))[a]
    pinm[nz - 1] = (U[nz - 1] - U[nz - 2]) / (pk(nz) - pk(nz - 1))

    # ---- :204-265 ----
    srcs = dict(uu=uuh, vv=vvh, tt=tth, qv=qvh, pv=pvh, rho=rhoh, pplev=np.broadcast_to(akz[:, None, None], (nz, ny, nx)))
    out = {k: np.full((nz, ny, nx), np.nan, H) for k in srcs}
    for k, A in srcs.items():
        out[k][0] = take(A, llev)
        out[k][nz - 1] = A[nuvz - 1]
    top = U[nuvz - 1]
    rec["above_uv"] = 0
    margin = np.inf
    for iz in range(2, nz):
        h = height[iz - 1]
        above = h > top
        rec["above_uv"] += int(above.sum())
        for k in srcs:
            out[k][iz - 1][above] = out[k][nz - 1][above]
        for kz in range(2, nuvz + 1):
            a = ~above & (kz >= llev + 1)
            a[a] = (h > U[kz - 2][a]) & (h <= U[kz - 1][a])
            if not a.any():
                continue
            dz1 = h - U[kz - 2][a]
            dz2 = U[kz - 1][a] - h
            dz = dz1 + dz2
            for k, A in srcs.items():
                out[k][iz - 1][a] = (A[kz - 2][a] * dz2 + A[kz - 1][a] * dz1) / dz
    for iz in range(2, nz + 1):
        margin = min(margin, float(np.min(np.abs(height[iz - 1].astype(np.float64) - top.astype(np.float64)) / top.astype(np.float64))))
    rec["margin"] = margin

    # ---- :271-285 ----
    ww = state["ww"].get(slot)
    ww = np.zeros((nz, ny, nx), H) if ww is None else ww.copy()
    ww[0] = take(wwh, llev) * take(pinm, llev)
    ww[nz - 1] = wwh[nwz - 1] * pinm[nz - 1]
    rec["above_w"] = rec["w_top_swept"] = 0
    for iz in range(2, nz + 1):
        h = height[iz - 1]
        found = np.zeros((ny, nx), bool)
        for kz in range(2, nwz + 1):
            a = kz >= llev + 1
            a[a] = (h > U[kz - 2][a]) & (h <= U[kz - 1][a])
            if not a.any():
                continue
            found |= a
            dz1 = h - U[kz - 2][a]
            dz2 = U[kz - 1][a] - h
            dz = dz1 + dz2
            ww[iz - 1][a] = (wwh[kz - 2][a] * pinm[kz - 2][a] * dz2 + wwh[kz - 1][a] * pinm[kz - 1][a] * dz1) / dz
        if iz < nz:
            rec["above_w"] += int((~found).sum())
        else:
            rec["w_top_swept"] = int(found.sum())

    # ---- :291-297 ----
    rho = out["rho"]
    drhodz = np.empty((nz, ny, nx), H)
    drhodz[0] = (rho[1] - rho[0]) / (height[1] - height[0])
    for kz in range(2, nz):
        drhodz[kz - 1] = (rho[kz] - rho[kz - 2]) / (height[kz] - height[kz - 2])
    drhodz[nz - 1] = drhodz[nz - 2]
    out["drhodz"] = drhodz

    # ---- :308-359 (interior columns) ----
    sl = (slice(1, ny - 1), slice(1, nx - 1))
    cosf = M.cos((np.arange(ny).astype(H) * dy + ylat0) * pi180)[:, None]
    Li = llev[sl]
    kl = np.zeros(Li.shape, np.int64)
    cdz1 = np.full(Li.shape, np.nan, H); cdz2 = cdz1.copy(); cdz = cdz1.copy()
    JJ, II = np.meshgrid(np.arange(1, ny - 1), np.arange(1, nx - 1), indexing="ij")
    rec["carried"] = rec["carry_across"] = 0
    for iz in range(2, nz):
        h = height[iz - 1]
        ui = (out["uu"][iz - 1] * dxconst / cosf)[sl]
        vi = (out["vv"][iz - 1] * dyconst)[sl]
        found = np.zeros(Li.shape, bool)
        for kz in range(2, nz + 1):
            a = ~found & (kz >= Li + 1)
            lo, hi = U[kz - 2][sl], U[kz - 1][sl]
            a[a] = (h > lo[a]) & (h <= hi[a])
            if not a.any():
                continue
            found |= a
            cdz1[a] = h - lo[a]
            cdz2[a] = hi[a] - h
            cdz[a] = cdz1[a] + cdz2[a]
            kl[a] = kz - 1
        if iz == 2:
            rec["carry_across"] = int((~found).sum())
        rec["carried"] += int((~found & (kl > 0)).sum())
        ok = kl > 0
        ka = np.where(ok, kl, 1) - 1                  # 0-based index of level kl; klp = kl + 1
        with np.errstate(invalid="ignore"):
            dzdx1 = (U[ka, JJ, II + 1] - U[ka, JJ, II - 1]) / H(2.)
            dzdx2 = (U[ka + 1, JJ, II + 1] - U[ka + 1, JJ, II - 1]) / H(2.)
            dzdx = (dzdx1 * cdz2 + dzdx2 * cdz1) / cdz
            dzdy1 = (U[ka, JJ + 1, II] - U[ka, JJ - 1, II]) / H(2.)
            dzdy2 = (U[ka + 1, JJ + 1, II] - U[ka + 1, JJ - 1, II]) / H(2.)
            dzdy = (dzdy1 * cdz2 + dzdy2 * cdz1) / cdz
            add = dzdx * ui + dzdy * vi
        add = np.where(ok, add, H(np.nan))
        ww[iz - 1][sl] = ww[iz - 1][sl] + add
    assert ww.dtype == H

    # ---- :366-494 ----
    uupol = np.zeros((nz, ny, nx), H); vvpol = np.zeros((nz, ny, nx), H)
    ic = nx // 2 - 1
    xl = xlon0 + np.arange(nx).astype(H) * dx
    rec["pole_vv"] = {}
    for south, on in ((False, nglobal), (True, sglobal)):
        if not on:
            continue
        north_map, south_map = (np.asarray(p).astype(H) for p in polemaps)
        if south:
            rows = range(0, min(ny - 1, int((H(SWITCHSOUTH) - ylat0) / dy) + 3) + 1)
            jpole, jnext = 0, 1
        else:
            rows = range(max(0, int((H(SWITCHNORTH) - ylat0) / dy) - 2), ny)
            jpole, jnext = ny - 1, ny - 2
        for jy in rows:
            ylat = ylat0 + H(jy) * dy
            for iz in range(nz):
                uupol[iz, jy], vvpol[iz, jy] = _cc2gll(M, south_map if south else north_map, ylat, xl, out["uu"][iz, jy], out["vv"][iz, jy])
        signs = []
        for iz in range(nz):
            xlon = xlon0 + H(ic) * dx
            xlonr = xlon * pi / H(180.)
            uc, vc = out["uu"][iz, jpole, ic], out["vv"][iz, jpole, ic]
            ffpol = np.sqrt(uc * uc + vc * vc)
            signs.append(int(np.sign(vc)))
            if vc < H(0.):
                ddpol = M.atan(uc / vc) + xlonr if south else M.atan(uc / vc) - xlonr
            elif vc > H(0.):
                ddpol = pi + M.atan(uc / vc) - xlonr       # :389 and :456 (GFS: - xlonr in the south too)
            else:
                ddpol = pi / H(2.) - xlonr
            ddpol = H(ddpol)
            if ddpol < H(0.):
                ddpol = H(2.0) * pi + ddpol
            if ddpol > H(2.0) * pi:
                ddpol = ddpol - H(2.0) * pi
            xlon = H(180.0)
            xlonr = xlon * pi / H(180.)
            if south:
                uuaux = +ffpol * H(M.sin(xlonr - ddpol)); vvaux = -ffpol * H(M.cos(xlonr - ddpol))
            else:
                uuaux = -ffpol * H(M.sin(xlonr + ddpol)); vvaux = -ffpol * H(M.cos(xlonr + ddpol))
            up, vp = _cc2gll(M, north_map, H(-90.0) if south else H(90.0), np.array([xlon], H), np.array([uuaux], H), np.array([vvaux], H))
            uupol[iz, jpole, :] = up[0]
            vvpol[iz, jpole, :] = vp[0]
            ww[iz, jpole, :] = np.cumsum(ww[iz, jnext, :], dtype=H)[-1] / H(nx)
        rec["pole_vv"]["south" if south else "north"] = signs
    state["ww"][slot] = ww.copy()
    out["ww"] = ww
    out["uupol"], out["vvpol"] = uupol, vvpol
    for k, v in out.items():
        assert v.dtype == H, k
    rec["masked"] = int(np.isnan(ww).sum())
    res = {k: v.astype(np.float64) for k, v in out.items()}
    res["height"] = height.astype(np.float64)
    res["nmixz"] = int(state["nmixz"])
    return res, rec


def run_case(kw, phases, kind, polemaps=None):
    """The three calls of a test case: slot 1 with init, slot 2, slot 1 again; kw = synthetic.gfs_levels() arguments without
    phase.  Returns [(fields, rec)] * 3."""
    from flexpart_amd import synthetic as syn
    st = new_state()
    outs = []
    for n, (slot, ph) in enumerate(zip((1, 2, 1), phases)):
        m = syn.gfs_levels(**kw, phase=ph)
        outs.append(vtgfs_ref(m, kind, st, slot, init=(n == 0), polemaps=polemaps))
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# the test cases (tests/test_verttransform_gfs.py, tests/golden/make_vtgfs_golden.py) and the conditions their inputs meet
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "flat": dict(nx=26, ny=22, nz=14, global_grid=False, polar=False, terrain=0.0),
    "terrain": dict(nx=70, ny=20, nz=16, global_grid=True, polar=True, terrain=51000.0),
    "cap": dict(nx=12, ny=10, nz=6, global_grid=False, polar=False, terrain=12500.0),
}
PHASES = (0, 9, 4)          # slot 1 with init, slot 2, slot 1 again


def case_polemaps(kw, kind):
    if not kw["polar"]:
        return None
    from flexpart_amd import synthetic as syn
    from oracle import oracle as orc
    g = syn.gfs_levels(**kw)["geom"]
    n, s, _, _ = orc.polemaps(g[0], g[1], g[3], kind)
    return n, s


def llev_steps_unmasked(llev, ww):
    """For x and y and both directions: is there an interior column whose neighbour's llev is larger / smaller and which has a
    ww cell of z levels 2..nz-1 that is not masked?  Returns {("x", +1): bool, ...}."""
    ny, nx = llev.shape
    free = (~np.isnan(ww[1:-1])).any(axis=0)[1:-1, 1:-1]
    c = llev[1:-1, 1:-1]
    nb = {"x": (llev[1:-1, 2:], llev[1:-1, :-2]), "y": (llev[2:, 1:-1], llev[:-2, 1:-1])}
    res = {}
    for ax, (p, q) in nb.items():
        res[(ax, +1)] = bool((free & ((p > c) | (q > c))).any())
        res[(ax, -1)] = bool((free & ((p < c) | (q < c))).any())
    return res


def check_conditions(case, kw, outs):
    """The conditions the issue of this feature sets for the inputs, from the restatement's record of the three calls (outs =
    run_case(..)).  Raises AssertionError naming the condition."""
    from flexpart_amd import synthetic as syn
    nz = kw["nz"]
    for n, (f, rec) in enumerate(outs):
        cells = f["ww"].size
        tag = f"{case} call {n}: "
        assert rec["carry_across"] == 0, tag + "a column would carry a slope bracket across columns"
        assert rec["margin"] >= 1e-6, tag + f"an above-the-top decision is closer than 1e-6 ({rec['margin']:.3e})"
        nlev = int((rec["llev_hist"] > 0).sum())
        if case == "flat":
            assert rec["masked"] == 0 and rec["above_uv"] == 0 and rec["above_w"] == 0 and nlev <= 2, tag + str(rec["masked"])
        else:
            assert rec["masked"] <= cells // 10, tag + f"{rec['masked']} of {cells} ww cells masked"
        if case == "terrain":
            assert nlev >= 5, tag + f"llev takes {nlev} values"
            for k in ("above_uv", "above_w", "tv_big", "tv_small", "carried"):
                assert rec[k] > 0, tag + k + " = 0"
            for pole in ("north", "south"):
                s = set(rec["pole_vv"][pole])
                assert 1 in s and -1 in s, tag + f"vv on the {pole} pole row has one sign only"
            st = llev_steps_unmasked(rec["llev"], f["ww"])
            assert all(st.values()), tag + f"llev steps that occur unmasked: {st}"
        if case == "cap":
            m = syn.gfs_levels(**kw, phase=PHASES[n])
            assert rec["llev_hist"][nz - 2] > 0 and (m["ps"] < m["akz"][nz - 3]).any(), tag + "llev does not hit its cap nuvz-2"
            assert (m["ps"] < m["akz"][nz - 4]).any()
