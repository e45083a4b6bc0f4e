"""numpy restatement of calcpv.f90:42-313 and calcpv_nests.f90 (the same algorithm with the nest's geometry and no global
flags) in a given real kind, vectorised over the horizontal grid.  Besides pvh it keeps a record of every decision:

  code[n][kl][jy][ix]  for the four neighbours n = x-, x+, y-, y+ of the search for the theta surface:
                       0 not searched (pole row), 1 bracket found upward at the first test, 2 upward at a later test,
                       3 downward, 4 search exhausted (label 21 / 51: kch >= nlck)
  tie[kl][jy][ix]      some bracket of the point took dt < eps (weights 0.5 / 0.5)
  margin[kl][jy][ix]   the smallest relative distance |theta - th| / |theta| over all bracket endpoints the point tested that
                       are not the same array element as theta, and |dt - eps| / eps where dt was formed: how far the point
                       is from taking another path.  A pole row has the smallest margin of the ring it averages.

Inputs: a synthetic.calcpv_case() dict (compact [nz][ny][nx] float64 arrays, geom = dx, dy, xlon0, ylat0 of the grid the
routine runs on, globalflags = xglobal, nglobal, sglobal)."""
import numpy as np

CODES = {"none": 0, "up_first": 1, "up_later": 2, "down": 3, "exhausted": 4}
KINDS = {"r4": np.float32, "r8": np.float64}


def _spiral(H, TH, W, JJ, II, own, theta, kl, nuvz, nlck, active, rec):
    """calcpv.f90:133-190 for every point of level kl (1-based) at once: the neighbour column of point (jy,ix) is
    (JJ,II); `own` marks points whose neighbour column is their own (domain edge).  Returns val, code."""
    eps = H(1.e-5)
    shape = theta.shape
    kup = np.full(shape, kl - 1, np.int64)
    kdn = np.full(shape, kl, np.int64)
    kch = np.zeros(shape, np.int64)
    val = np.zeros(shape, H)
    code = np.zeros(shape, np.int8)
    active = active.copy()
    th64 = np.abs(theta.astype(np.float64))

    def test(mask, kk, found_code):
        kc = np.where(mask, kk, 1)
        thdn, thup = TH[kc - 1, JJ, II], TH[kc, JJ, II]
        for lev, th in ((kc, thdn), (kc + 1, thup)):                   # the margin of both endpoints, unless it is theta itself
            m = mask & ~(own & (lev == kl))
            d = np.abs(theta.astype(np.float64) - th.astype(np.float64)) / th64
            rec["margin"][kl - 1][m] = np.minimum(rec["margin"][kl - 1][m], d[m])
        br = mask & (((thdn >= theta) & (thup <= theta)) | ((thdn <= theta) & (thup >= theta)))
        dt1, dt2 = np.abs(theta - thdn), np.abs(theta - thup)
        dt = dt1 + dt2
        dm = np.abs(dt.astype(np.float64) - float(eps)) / float(eps)
        rec["margin"][kl - 1][br] = np.minimum(rec["margin"][kl - 1][br], dm[br])
        small = dt < eps
        rec["tie"][kl - 1] |= br & small
        dt1 = np.where(small, H(0.5), dt1); dt2 = np.where(small, H(0.5), dt2); dt = np.where(small, H(1.0), dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (W[kc - 1, JJ, II] * dt2 + W[kc, JJ, II] * dt1) / dt
        val[br] = v[br]
        code[br] = found_code[br] if isinstance(found_code, np.ndarray) else found_code
        return br

    while active.any():
        kup[active] += 1                                               # 40
        fail = active & (kch >= nlck)
        code[fail] = CODES["exhausted"]
        active &= ~fail
        up = active & (kup < nuvz)
        kch[up] += 1
        active &= ~test(up, kup, np.where(kch == 1, CODES["up_first"], CODES["up_later"]).astype(np.int8))
        kdn[active] -= 1                                               # 41
        dn = active & (kdn >= 1)
        kch[dn] += 1
        active &= ~test(dn, kdn, CODES["down"])
    return val, code


def calcpv_ref(c, kind):
    H = KINDS[kind]
    nx, ny, nuvz = (int(v) for v in c["grid"])
    dx, dy, ylat0 = H(c["geom"][0]), H(c["geom"][1]), H(c["geom"][3])
    xglobal, nglobal, sglobal = (bool(v) for v in c["globalflags"])
    akz, bkz, ps = (np.asarray(c[k]).astype(H) for k in ("akz", "bkz", "ps"))
    tth, uuh, vvh = (np.asarray(c[k]).astype(H) for k in ("tth", "uuh", "vvh"))
    pi, r_earth = H(3.14159265), H(6.371e6)
    nlck = nuvz // 3
    ppml = akz[:, None, None] + bkz[:, None, None] * ps[None]
    ppmk = np.power(H(100000.) / ppml, H(0.286))
    TH = tth * ppmk
    assert ppml.dtype == H and TH.dtype == H
    jy = np.arange(ny)[:, None] + np.zeros((1, nx), np.int64)
    ix = np.arange(nx)[None, :] + np.zeros((ny, 1), np.int64)
    phi = (ylat0 + np.arange(ny).astype(H) * dy) * pi / H(180.)
    f = (H(0.00014585) * np.sin(phi))[:, None]
    tanphi, cosphi = np.tan(phi)[:, None], np.cos(phi)[:, None]
    assert f.dtype == H and tanphi.dtype == H
    # the virtual neighbours (:64-100)
    jyvp, jyvm = np.minimum(jy + 1, ny - 1), np.maximum(jy - 1, 0)
    jumpy = np.where((jy == 0) | (jy == ny - 1), 1, 2)
    if sglobal:
        jyvm = np.where(jy == 1, 1, jyvm); jumpy = np.where(jy == 1, 1, jumpy)
    if nglobal:
        jyvp = np.where(jy == ny - 2, ny - 2, jyvp); jumpy = np.where(jy == ny - 2, 1, jumpy)
    if xglobal:
        ivrm = np.where(ix - 1 < 0, ix - 1 + (nx - 1), ix - 1)
        ivrp = np.where(ix + 1 >= nx, ix + 1 - nx + 1, ix + 1)
        jumpx = np.full((ny, nx), 2)
    else:
        ivrm, ivrp = np.maximum(ix - 1, 0), np.minimum(ix + 1, nx - 1)
        jumpx = np.where((ix == 0) | (ix == nx - 1), 1, 2)
    rows = np.ones((ny, nx), bool)
    if sglobal:
        rows &= jy != 0
    if nglobal:
        rows &= jy != ny - 1
    rec = dict(margin=np.full((nuvz, ny, nx), np.inf), tie=np.zeros((nuvz, ny, nx), bool), code=np.zeros((4, nuvz, ny, nx), np.int8))
    pvh = np.zeros((nuvz, ny, nx), H)
    for kl in range(1, nuvz + 1):
        theta = TH[kl - 1]
        klvrp, klvrm = min(kl + 1, nuvz), max(kl - 1, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            dthetadp = (TH[klvrp - 1] - TH[klvrm - 1]) / (ppml[klvrp - 1] - ppml[klvrm - 1])
        vx, cx = zip(*[_spiral(H, TH, vvh, jy, iv, iv == ix, theta, kl, nuvz, nlck, rows, rec) for iv in (ivrm, ivrp)])
        uy, cy = zip(*[_spiral(H, TH, uuh, jv, ix, jv == jy, theta, kl, nuvz, nlck, rows, rec) for jv in (jyvm, jyvp)])
        for n, cc in enumerate(cx + cy):
            rec["code"][n, kl - 1] = cc
        ex = CODES["exhausted"]
        vx = [np.where(cc == ex, vvh[kl - 1], v) for v, cc in zip(vx, cx)]
        uy = [np.where(cc == ex, uuh[kl - 1], v) for v, cc in zip(uy, cy)]
        jux = jumpx - (cx[0] == ex) - (cx[1] == ex)
        juy = jumpy - (cy[0] == ex) - (cy[1] == ex)
        dvdx = np.where(jux > 0, (vx[1] - vx[0]) / np.maximum(jux, 1).astype(H) / (dx * pi / H(180.)),
                        (vvh[kl - 1][jy, ivrp] - vvh[kl - 1][jy, ivrm]) / jumpx.astype(H) / (dx * pi / H(180.)))
        dudy = np.where(juy > 0, (uy[1] - uy[0]) / np.maximum(juy, 1).astype(H) / (dy * pi / H(180.)),
                        (uuh[kl - 1][jyvp, ix] - uuh[kl - 1][jyvm, ix]) / jumpy.astype(H) / (dy * pi / H(180.)))
        with np.errstate(invalid="ignore", divide="ignore"):
            val = dthetadp * (f + (dvdx / cosphi - dudy + uuh[kl - 1] * tanphi) / r_earth) * H(-1.e6) * H(9.81)
        assert val.dtype == H
        pvh[kl - 1] = np.where(rows, val, H(0.))
        for pole, ring, on in ((0, 1, sglobal), (ny - 1, ny - 2, nglobal)):    # :288-313, summed in the reference's order
            if on:
                pvh[kl - 1, pole, :] = np.cumsum(pvh[kl - 1, ring, :], dtype=H)[-1] / H(nx)
                rec["margin"][kl - 1, pole, :] = rec["margin"][kl - 1, ring, :].min()
    rec["pvh"] = pvh.astype(np.float64)
    rec["theta"] = TH.astype(np.float64)
    rec["jux0"] = (rec["code"][0] == CODES["exhausted"]) & (rec["code"][1] == CODES["exhausted"])
    rec["juy0"] = (rec["code"][2] == CODES["exhausted"]) & (rec["code"][3] == CODES["exhausted"])
    return rec


def level_error(got, gold):
    """|got - gold| relative to the largest |gold| of the same model level: [nz][ny][nx]"""
    scale = np.abs(gold).reshape(gold.shape[0], -1).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)[:, None, None]
    return np.abs(np.asarray(got, np.float64) - gold) / scale
